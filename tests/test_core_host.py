"""tests/core_cases.py without a GPU: the coverage assertions (the static tables reach every cell that the restated dispatch of
csrc/hipk_core.hip can choose; what they do not reach is spelt out with the reason), and every case whose contract the
plain-C oracle implements, on the oracle: copies, hipk_memset0, hipk_d2d, the mirror contents after a reduction and after
hipk_publish_results, the fused product's dot and the other second-stage producers, hipk_sym_eig, hipk_larnv_uniform11.
Where the oracle is a stub (core_cases.ORACLE_SAME) no device semantics are asserted on it."""
import ctypes as C

import numpy as np
import pytest

from kernel_harness import Host
import core_cases as B


# ---- coverage of the tables -------------------------------------------------------------------------------------------
def test_fin_block_for_and_regions_restated():
    assert [B.fin_block_for(n) for n in (1, 1024, 1025, 2048, 2049, 100000)] == [256, 256, 512, 512, 1024, 1024]
    # the loop starts only above three block widths, and a thread that looped has at most three terms left
    for nb in (1, 8, 768, 769, 776, 1024, 1025, 1536, 1537, 2048, 2049, 3072, 3073, 4104, 7168, 7169):
        nt, looped, rounds, live = B.fin_regions(nb)
        assert (looped == "none") == (nb <= 3 * nt) and (rounds >= 2) == (nb > 7 * nt) and live <= {0, 1, 2, 3}
        # every partial is added exactly once: the rounds and the live tail terms of all threads add up to nblocks
        total = 0
        for t in range(nt):
            r = 0 if nb <= t + 3 * nt else -(-(nb - t - 3 * nt) // (4 * nt))
            total += 4 * r + sum(1 for j in range(3) if t + 4 * nt * r + j * nt < nb)
        assert total == nb


def test_scaled_cases_reach_every_second_stage_cell(built):
    cells, lives, classes = {}, {}, {}
    for c in B.SCALED_CASES:
        assert B.scaled_gx(c["ntiles"]) == c["gx"]
        nt, looped, rounds, live = B.fin_regions(c["gx"])
        cells.setdefault((nt, looped), set()).add((c["dt"], c["gx"]))
        lives.setdefault(nt, set()).update(live)
        assert rounds <= 1
        if c["ntiles"] % 8:
            classes.setdefault(nt, set()).add(c["dt"])
    assert set(cells) == B.FIN_CELLS and len(B.FIN_CELLS) == 9
    for cell, who in cells.items():
        assert {dt for dt, _ in who} == set(B.TYPES), cell
    # the sizes the issue names, in both types; one ntiles % 8 != 0 per block-size class and type
    assert {c["gx"] for c in B.SCALED_CASES} == {8, 768, 776, 1024, 1032, 1544, 2048, 2056, 3080, 4104}
    assert classes == {256: set(B.TYPES), 512: set(B.TYPES), 1024: set(B.TYPES)}
    # every number of live tail terms at every block size where the geometry allows it
    assert lives == {256: {0, 1, 3}, 512: {0, 2, 3}, 1024: {0, 1, 2, 3}}
    where = {gx: B.fin_regions(gx)[:2] for gx, _ in B.SCALED_TILES}
    assert where == {8: (256, "none"), 768: (256, "none"), 776: (256, "some"), 1024: (256, "all"), 1032: (512, "none"), 1544: (512, "some"),
                     2048: (512, "all"), 2056: (1024, "none"), 3080: (1024, "some"), 4104: (1024, "all")}
    assert all(isinstance(r, str) and r for r in B.FIN_UNREACHABLE.values()) and len(B.FIN_UNREACHABLE) == 5
    assert B.NROWS_MAX * (2 * 12 + 4) < 32 << 20                 # the largest matrix: values, columns and row pointers


def test_scaled_matrices_are_cut_at_the_row_limit(built):
    for gx, ntiles in B.SCALED_TILES:
        plan = B.scaled_plan(dict(ntiles=ntiles))
        n = 256 * ntiles - 3
        assert plan.ntiles == ntiles and plan.tiles[-1] == n and plan.tiles[-1] - plan.tiles[-2] == 253, (gx, ntiles)
        assert (plan.halo_lo, plan.halo_hi) == (0, 0)


def test_other_layouts_have_at_least_two_partials_on_any_device():
    layouts = set()
    for c in B.OMAJOR_CASES + B.STRIDED_CASES:
        assert B.min_partials(c, num_cu=1) >= 2, B.case_id(c)
        assert B.fin_block_for(B.min_partials(c, num_cu=256)) == 256
        layouts.add((B.fin_layout_of(c), c["dt"]))
    layouts |= {(B.fin_layout_of(c), c["dt"]) for c in B.SCALED_CASES}
    assert layouts == {(l, dt) for l in ("partial-major nout=1", "o-major", "strided pstride!=nout") for dt in B.TYPES}
    assert {c["nx"] for c in B.OMAJOR_CASES if c["ep"] == "project"} == {1, 3}
    for c in B.STRIDED_CASES:
        assert 2 * c["nb"] + 2 * c["L"] + 1 != 1                 # pstride = nsl against nout = 1


def test_copy_cases_reach_every_route():
    routes = B.copy_routes(B.COPY_CASES)
    assert set(routes) == B.COPY_ROUTES_WANTED, (set(routes) ^ B.COPY_ROUTES_WANTED)
    by = dict(zip(map(B.copy_id, B.COPY_CASES), routes))
    assert len(by) == len(B.COPY_CASES)
    assert by["lib-65536-h0-d0"] == ("copy kernel", "one pass", "full blocks") and by["lib-65540-h0-d0"] == ("copy kernel", "grid-stride", "ragged block")
    assert by["lib-6-h0-d0"] == ("runtime", "lib: bytes % 4") and by["lib-1048580-h0-d0"] == ("runtime", "lib: over 1 MiB")
    assert by["lib-1024-h2-d0"][1] == "lib: pinned side unaligned" and by["lib-1024-h0-d2"][1] == "lib: device side unaligned"
    assert by["pageable-65537-h1-d3"] == ("staged", "grow", "one chunk") and by["pageable-100-h1-d3"] == ("staged", "reuse", "one chunk")
    assert by[f"pageable-{(32 << 20) + 4099}-h1-d3"] == ("staged", "grow", "chunks, ragged last")
    for n in (4, 8, 1020, 65536, 65540, 1048576):                # the copy-kernel sizes with either side 4 bytes in
        assert {by[f"lib-{n}-h{h}-d{d}"][0] for h, d in ((0, 0), (4, 0), (0, 4))} == {"copy kernel"}
    assert all(isinstance(r, str) and r for r in B.COPY_UNREACHABLE.values())
    assert not set(B.COPY_UNREACHABLE) & set(routes)


def test_what_the_oracle_cannot_tell_apart_is_named():
    assert set(B.ORACLE_SAME) == {"hipk_seq_issued", "hipk_wait_seq / hipk_wait_results", "hipk_skip_next_flag", "hipk_publish_results", "mirror bound",
                                  "hipk_is_device_ptr", "hipk_prof_*", "copy routing", "second stage", "hipk_sym_eig n > 64"}
    lib = B.declare(Host().lib)
    ctx = C.c_void_p()
    assert lib.hipk_ctx_create(C.byref(ctx), None) == 0
    assert lib.hipk_seq_issued(ctx) == 0 and lib.hipk_wait_seq(ctx, 7) == 0 and lib.hipk_wait_results(ctx) == 0
    assert lib.hipk_is_device_ptr(None) == 0 and lib.hipk_is_device_ptr(C.c_void_p(np.zeros(1).ctypes.data)) == 1
    lib.hipk_ctx_destroy(ctx)


# ---- the cases the oracle implements ----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", B.SCALED_CASES, ids=B.case_id)
def test_oracle_scaled_dot(built, c):
    rep = B.run_cases(Host, [c])
    assert not rep.fails, "\n".join(rep.fails[:20])


@pytest.mark.parametrize("c", B.OMAJOR_CASES + B.STRIDED_CASES, ids=B.case_id)
def test_oracle_other_second_stage_producers(built, c):
    rep = B.run_cases(Host, [c])
    print(rep.summary())
    assert not rep.fails, "\n".join(rep.fails[:20])


@pytest.mark.parametrize("dt", B.TYPES, ids=B.TNAME.get)
@pytest.mark.parametrize("nx", [1, 3])
def test_oracle_mirror_after_a_reduction(built, dt, nx):
    for off in (0, 7, 40 - nx):
        side = Host()
        B.proto_flagged(side, dt, nx, off)
        side.close()


@pytest.mark.parametrize("count", B.PUBLISH_COUNTS)
def test_oracle_mirror_after_publish(built, count):
    side = Host()
    B.proto_publish(side, count)
    side.close()


def test_oracle_copies_and_utilities(built):
    side = Host()
    rig = B.CopyRig(side, 1 << 21)
    for c in B.COPY_CASES:
        if c["n"] <= 1 << 21:
            B.run_copy(side, rig, c, foreign=np.empty(c["n"] + 2 * B.PAD + 8, np.uint8) if c["kind"] == "foreign" else None)
    rig.close()
    for n in B.UTIL_SIZES:
        B.run_d2d(side, n)
        B.run_memset0(side, n)
    side.close()


@pytest.mark.parametrize("n", B.EIG_N)
@pytest.mark.parametrize("kind", B.EIG_KINDS)
def test_oracle_sym_eig(built, kind, n):
    side = Host()
    B.run_sym_eig(side, kind, n)
    side.close()


@pytest.mark.parametrize("dt", B.TYPES, ids=B.TNAME.get)
def test_oracle_larnv(built, dt):
    side = Host()
    for seed in B.LARNV_SEEDS:
        for n in B.LARNV_N + [0]:
            B.run_larnv(side, dt, seed, n)
    side.close()
