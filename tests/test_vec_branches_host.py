"""Every case of tests/vec_branch_cases.py on the plain-C oracle (oracle/hipk_cpu.c, oracle/hipk_cpu_complex.c) against the
longdouble references written from the header: pins the oracle to an independent statement of each operation, of the
denominator guard and of the return codes, and holds it to the bit-for-bit identities the header promises.  Plus the coverage
assertions: the static tables reach every instantiation of csrc/hipk_vec.hip in scope and every row / column cell that exists."""
import numpy as np
import pytest

from kernel_harness import Host
import vec_branch_cases as V

GROUPS = V.groups()


@pytest.mark.parametrize("gid,cases", GROUPS, ids=[g for g, _ in GROUPS])
def test_oracle_against_longdouble_reference(built, gid, cases):
    rep = V.run_cases(Host, cases)
    print(f"{gid}: {rep.summary()}")
    assert not rep.fails, f"{gid}: {rep.summary()}\n" + "\n".join(rep.fails[:20])


def test_no_case_is_left_out_of_a_group():
    assert sum(len(cs) for _, cs in GROUPS) == len(V.CASES) + len(V.DROP) + len(V.RC)


def test_case_tables_cover_every_instantiation():
    """19 real kernels x 2 types + zjacobi_kernel x 2 = 40 (copy_cols_kernel and fill_kernel are out of scope)"""
    have = {b[:-1] for c in V.CASES for b in V.branch_of(c)}
    real = {b for b in have if b[0] != "zjacobi_kernel"}
    print(sorted(map(str, have)))
    assert len(have) == 40 and len(real) == 38 and len({(b[0],) + b[2:] for b in real}) == 19
    assert {b for b in have if b[0] == "zjacobi_kernel"} == {("zjacobi_kernel", "c64"), ("zjacobi_kernel", "c32")}
    for k in ("axpy_proj_dot_jacobi_kernel", "qmr_update_dir_kernel"):
        assert {b[1:] for b in have if b[0] == k} == {(t, f) for t in ("f64", "f32") for f in (False, True)}


def test_launches_of_the_chunked_kernels():
    """c0 of every launch: 65 and 129 columns of a utility make a second and a third launch, 9 / 16 / 17 / 64 of the passes with the
    diagonal a second to an eighth"""
    c0s = {}
    for c in V.CASES:
        for b in V.branch_of(c):
            c0s.setdefault(V.kernel_key(b), set()).add(b[-1])
    for k in ("scale_kernel", "axpy_kernel", "xpay_kernel", "gather_kernel", "residual_kernel"):
        assert c0s[k] == {0, 64, 128}, k
    for k in ("qmr_update_jacobi_kernel", "axpy_proj_dot_jacobi_kernel", "qmr_update_dir_kernel"):
        assert c0s[k] == set(range(0, 64, 8)), k
    for k, v in c0s.items():
        assert v == {0} or "next-chunk" not in V.NO_CELL.get(k, {}), k


def test_case_tables_cover_every_cell_that_exists():
    rows, cols = {}, {}
    for c in V.CASES:
        r, cc = V.cells_of(c)
        for b in V.branch_of(c):
            rows.setdefault((V.kernel_key(b), b[1]), set()).add(r)
            cols.setdefault((V.kernel_key(b), b[1]), set()).add(cc)
    assert len(rows) == 40
    for (k, t), have in rows.items():
        none = V.NO_CELL.get(k, {})
        assert all(isinstance(v, str) and v for v in none.values())
        assert have == set(V.ROW_CELLS) - set(none), (k, t, have)
        assert cols[(k, t)] == set(V.COL_CELLS) - set(none), (k, t, cols[(k, t)])
    assert set(V.NO_CELL) <= {k for k, _ in rows}
    assert {k for k, v in V.NO_CELL.items() if "next-chunk" in v} == {k for (k, _), v in cols.items() if "next-chunk" not in v}


def test_column_counts_of_the_issue():
    for ep, spec in V.EPS.items():
        for dt in V.RTYPES:
            assert {c["nx"] for c in V.CASES if c["ep"] == ep and c["dt"] == dt and not c.get("cap")} == set(spec[4]), ep
    for dt in V.ZTYPES:
        assert {c["nx"] for c in V.CASES if c["dt"] == dt and not c.get("cap")} == {1, 3, 64}
    assert V.gather_perm(1) == [1] and V.gather_perm(5) == [5, 4, 3, 2, 5]
    for ep in V.EPS:
        for dt in V.RTYPES:
            assert {c["m"] for c in V.CASES if c["ep"] == ep and c["dt"] == dt and not c.get("cap")} >= set(V.M_ROWS), ep


def test_every_entry_point_has_every_flavour_on_every_type():
    for ep in V.EPS:
        for dt in V.RTYPES + (V.ZTYPES if ep == "jacobi" else []):
            assert {c["flavour"] for c in V.CASES if c["ep"] == ep and c["dt"] == dt} == set(V.FLAVOURS), (ep, dt)
    for fl in V.FLAVOURS:                       # the flavours are what they are called
        for dt in V.RTYPES:
            for m in (1, 64, 65, 257):
                op = V._lay(dt, m, 2, fl, 1)
                assert V.is_vec(dt, op) == (fl == "vec") and (fl != "odd" or op.ld % 2 == 1) and (fl != "shift" or op.shift == 1)
                assert op.off >= V.GUARD and op.ld >= m


def test_guard_rows_of_every_entry_point_with_a_guard():
    guarded = [ep for ep, spec in V.EPS.items() if spec[8]]
    assert sorted(guarded) == ["axpy_proj_dot_jacobi", "axpy_proj_dot_jacobi_dev", "jacobi", "qmr_update_dir", "qmr_update_dir_dev", "qmr_update_jacobi"]
    for ep in guarded:
        for dt in V.RTYPES + (V.ZTYPES if ep == "jacobi" else []):
            mine = [c for c in V.CASES if c["ep"] == ep and c["dt"] == dt]
            assert {cls for c in mine for _, _, cls in V.guard_rows_of(c)} == set(V.GUARD_ROWS), (ep, dt)
            assert all(len(V.guard_rows_of(c)) >= min(5, c["m"]) for c in mine if not c.get("mind0"))
            assert sum(1 for c in mine if c.get("mind0")) == 1 and sum(1 for c in mine if c.get("noshift")) == 1
            assert sum(1 for c in mine if c.get("nanrow")) == (1 if ep == "jacobi" else 0)
    # the rows are what they are called, the clamp decision is the same in every precision, and min_denominator = 0 meets no zero
    for c in V.CASES:
        if not V.EPS[c["ep"]][8] or c["m"] > 5000:
            continue
        ops, s, d = V.build(c)
        diag = d["diag"][0].real.astype(np.float64)
        ok = ~np.isnan(diag)
        assert np.all(diag[ok] * 256 == np.round(diag[ok] * 256)) and np.all(np.abs(diag[ok]) < 256) and np.all(s["shift0"] * 256 == np.round(s["shift0"] * 256))
        for row, col, cls in V.guard_rows_of(c):
            assert diag[row] - s["shift0"][col] == V.GUARD_DEN[cls], V.case_id(c)
        if c.get("mind0"):
            assert s["mind"] == 0.0 and np.all(diag[:, None] - s["shift0"][None, :] != 0.0)
        assert (s["shift"] is None) == bool(c.get("noshift"))
    g = V.GUARD_DEN
    assert g["zero"] == 0 and 0 < g["pos-small"] < V.MIND and -V.MIND < g["neg-small"] < 0 and abs(g["equal"]) == V.MIND and g["above"] == V.MIND + 2.0 ** -8


def test_drop_classes_in_first_middle_and_last_column():
    for dt in V.RTYPES:
        mine = [c for c in V.DROP if c["dt"] == dt]
        assert {c["nx"] for c in mine} == {1, 5, 8}
        for cls in V.DROP_CLASSES + ("live",):
            where = {("first" if i == 0 else "last" if i == c["nx"] - 1 else "middle") for c in mine if c["nx"] > 1 for i, k in enumerate(c["classes"]) if k == cls}
            assert where == {"first", "middle", "last"}, cls
            assert any(c["classes"] == (cls,) for c in mine)
        assert any("live" not in c["classes"] and c["nx"] > 1 for c in mine)
        for c in mine:                                       # tri and rho_prev put every column in its class
            tri, rho = V.drop_tri(c, V._rng(c))
            alpha, bad = V.qmr_alpha(tri, rho, c["nx"])
            assert bad.tolist() == [k != "live" for k in c["classes"]] and np.all(np.isfinite(tri[:c["nx"]]))
            with np.errstate(all="ignore"):
                sigma = tri[c["nx"]:2 * c["nx"]] - tri[:c["nx"]] * tri[2 * c["nx"]:]
                a = rho / sigma
            for i, k in enumerate(c["classes"]):
                assert {"sigma0": sigma[i] == 0, "sigma_inf": np.isinf(sigma[i]), "sigma_nan": np.isnan(sigma[i]),
                        "alpha_tiny": 0 < abs(a[i]) < V.MACH_EPS, "rho0": a[i] == 0 and sigma[i] != 0, "alpha_huge": np.isfinite(a[i]) and abs(a[i]) > 1 / V.MACH_EPS,
                        "alpha_inf": np.isinf(a[i]) and np.isfinite(sigma[i]), "live": True}[k], (V.case_id(c), i)


def test_return_code_cases_of_the_issue():
    def has(ep, dt, kind, rc):
        return any(c["ep"] == ep and c["dt"] == dt and c["kind"] == kind and c["rc"] == rc for c in V.RC)
    for dt in V.RTYPES:
        assert all(has(ep, dt, "nx0", 0) for ep in V.EPS)
        assert all(has(ep, dt, "nx65", -1) for ep in V.RC_LIMIT64 + ("jacobi",))
        assert all(has(ep, dt, k, -1) for ep in V.DEV_EPS for k in ("nx9", "tri_null")) and has("qmr_update_dir_dev", dt, "ggr_null", -1)
    for dt in V.ZTYPES:
        assert has("jacobi", dt, "nx65", -1) and all(has(ep, dt, "complex", -44) for ep in V.RC_REAL_ONLY)


def test_sizes():
    for c in V.CASES + V.DROP + V.RC:
        cap = bool(c.get("cap"))
        assert cap == (c["m"] > 5000) and c["nx"] <= 129 and (c["nx"] < 64 or c["m"] <= 257)
        if cap:
            assert V.cells_of(c)[0] == "capped" and c["nx"] == (2 if c["ep"] == "triple" else 1)
            assert c["m"] == 1024 * V.EPS[c["ep"]][2] * V.NUM_CU + 1029
    assert V.NUM_CU == 256


def test_layouts_differ_within_a_case():
    for c in V.CASES + V.DROP + V.RC:
        if c["m"] > 5000:
            c = dict(c, m=c["m"] % 5000)          # the leading dimensions of a flavour differ by the same steps at every m
        lds = [op.ld for op in V.panels(c).values()]
        assert len(set(lds)) == len(lds), (V.case_id(c), lds)
        if c["ep"] in ("axpy_proj_dot", "axpy_dot", "qmr_update_dir", "qmr_update_jacobi"):
            assert V._scratch(c, V.panels(c)["G" if "G" in V.panels(c) else "X"], None).ld not in lds
