"""csrc/hipk_core.hip on the device (-m gpu): the cases of tests/core_cases.py through kernel_harness.Dev.
  A  the second stage in its three layouts, every (block size, loop region) cell through hipk_csr_matvec_scaled on the row tiles
  B  the pinned result mirror, the completion flag and the sequence numbers (hipk_ctx_set_mirror, hipk_wait_results,
     hipk_wait_seq, hipk_seq_issued, hipk_skip_next_flag, hipk_publish_results)
  C  hipk_h2d / hipk_d2h on every route, hipk_d2d, hipk_memset0, hipk_is_device_ptr, zero-byte allocations, the timer, the profiler
  D  hipk_sym_eig and hipk_larnv_uniform11 at the shapes tests/test_kernels_gpu.py leaves out
HIPK_NO_COPY_KERNEL is read once per process and stays untested: no test here starts a child process.  No test waits for a
flag that nobody publishes.  tests/test_core_host.py runs what the oracle implements and asserts the coverage of the tables."""
import ctypes as C
import math

import numpy as np
import pytest

from kernel_harness import Dev
import core_cases as B

pytestmark = pytest.mark.gpu
TID = B.TNAME.get


@pytest.fixture
def side(built):
    s = Dev()
    B.declare(s.lib)
    yield s
    s.close()


# ---- A. second stage ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", B.SCALED_CASES, ids=B.case_id)
def test_second_stage_partial_major(built, c):
    rep = B.run_cases(Dev, [c])
    assert not rep.fails, "\n".join(rep.fails[:20])


@pytest.mark.parametrize("c", B.OMAJOR_CASES + B.STRIDED_CASES, ids=B.case_id)
def test_second_stage_o_major_and_strided(built, c):
    rep = B.run_cases(Dev, [c])
    print(rep.summary())
    assert not rep.fails, "\n".join(rep.fails[:20])


# ---- B. mirror, flag, sequence numbers ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", B.TYPES, ids=TID)
@pytest.mark.parametrize("nx", [1, 3])
def test_flagged_reduction(side, dt, nx):
    for off in (0, 7, 40 - nx):
        B.proto_flagged(side, dt, nx, off)


@pytest.mark.parametrize("dt", B.TYPES, ids=TID)
@pytest.mark.parametrize("nx", [1, 3])
@pytest.mark.parametrize("where", ["separate", "one past the end"])
def test_unmirrored_output(side, dt, nx, where):
    B.proto_unmirrored(side, dt, nx, where)


@pytest.mark.parametrize("dt", B.TYPES, ids=TID)
def test_straddling_output_is_not_mirrored(side, dt):
    """An output range that starts inside the declared mirror and ends past it.  Before the range check in launch_finalize /
    hipk_make_fin / hipk_next_flag the second stage stored h[N] and h[N + 1] (and published a flag for them): this test failed
    on the changed sentinels.  The contract now: such a range is not mirrored at all."""
    B.proto_straddle(side, dt)


@pytest.mark.parametrize("dt", B.TYPES, ids=TID)
def test_wait_seq(side, dt):
    B.proto_wait_seq(side, dt)


@pytest.mark.parametrize("dt", B.TYPES, ids=TID)
def test_skip_next_flag(side, dt):
    B.proto_skip(side, dt)


@pytest.mark.parametrize("count", B.PUBLISH_COUNTS)
def test_publish_results(side, count):
    B.proto_publish(side, count)


def test_publish_results_declined(side):
    B.proto_publish_declined(side)


@pytest.mark.parametrize("dt", B.TYPES, ids=TID)
def test_ticket_reuse(side, dt):
    """The bound of the wait is not measured: an unpublished flag degrades to a drain after the spin limit, and only this
    printed time shows it."""
    worst = B.proto_tickets(side, dt)
    print(f"longest hipk_wait_results: {1e6 * worst:.1f} us")


@pytest.mark.parametrize("dt", B.TYPES, ids=TID)
def test_mirror_off(side, dt):
    B.proto_mirror_off(side, dt)


# ---- C. copies and utilities -------------------------------------------------------------------------------------------
def _foreign(n):
    import torch
    t = torch.empty(n + 2 * B.PAD + 8, dtype=torch.uint8, pin_memory=True)
    return t, t.numpy()


@pytest.mark.parametrize("kind", ["lib", "foreign"])
def test_copies_pinned(side, kind):
    cases = [c for c in B.COPY_CASES if c["kind"] == kind]
    rig = B.CopyRig(side, max(c["n"] for c in cases))
    try:
        for c in cases:
            keep, view = _foreign(c["n"]) if kind == "foreign" else (None, None)
            if kind == "foreign":
                assert side.lib.hipk_is_device_ptr(C.c_void_p(view.ctypes.data)) == 0
            B.run_copy(side, rig, c, foreign=view)
            side.lib.hipk_sync(side.ctx)
            del keep
    finally:
        rig.close()


def test_copies_pageable(side):
    """in the order of the table on this fresh context: the staging buffer grows, is reused, and a copy takes two chunks"""
    cases = [c for c in B.COPY_CASES if c["kind"] == "pageable"]
    assert B.copy_routes(cases)[0] == ("staged", "grow", "one chunk")
    rig = B.CopyRig(side, max(c["n"] for c in cases))
    try:
        for c in cases:
            B.run_copy(side, rig, c)
    finally:
        rig.close()


@pytest.mark.parametrize("n", B.UTIL_SIZES)
def test_d2d_and_memset0(side, n):
    B.run_d2d(side, n)
    B.run_memset0(side, n)


def test_is_device_ptr(side):
    lib = side.lib
    assert lib.hipk_is_device_ptr(None) == 0
    a = np.zeros(16)
    assert lib.hipk_is_device_ptr(C.c_void_p(a.ctypes.data)) == 0
    d = C.c_void_p()
    assert lib.hipk_malloc(side.ctx, 4096, C.byref(d)) == 0 and d          # the sticky error of the pageable query was cleared
    assert lib.hipk_is_device_ptr(d) == 1 and lib.hipk_is_device_ptr(C.c_void_p(d.value + 1001)) == 1
    h = C.c_void_p()
    assert lib.hipk_host_alloc(side.ctx, 4096, C.byref(h)) == 0
    assert lib.hipk_is_device_ptr(h) == 0
    keep, view = _foreign(1024)
    assert lib.hipk_is_device_ptr(C.c_void_p(view.ctypes.data)) == 0
    assert lib.hipk_free(side.ctx, d) == 0 and lib.hipk_host_free(side.ctx, h) == 0


def test_zero_byte_allocations(side):
    lib = side.lib
    d, h = C.c_void_p(), C.c_void_p()
    assert lib.hipk_malloc(side.ctx, 0, C.byref(d)) == 0 and d
    assert lib.hipk_host_alloc(side.ctx, 0, C.byref(h)) == 0 and h
    np.ctypeslib.as_array((C.c_uint8 * 8).from_address(h.value))[:] = B.ramp(8)
    assert lib.hipk_h2d(side.ctx, d, h, 8) == 0 and lib.hipk_memset0(side.ctx, d, 4) == 0
    assert lib.hipk_d2h(side.ctx, h, d, 8) == 0 and lib.hipk_sync(side.ctx) == 0
    assert np.ctypeslib.as_array((C.c_uint8 * 8).from_address(h.value)).tolist() == [0, 0, 0, 0] + B.ramp(8)[4:].tolist()
    assert lib.hipk_free(side.ctx, d) == 0 and lib.hipk_host_free(side.ctx, h) == 0


def test_timer(side):
    lib = side.lib
    t = side.arr(np.full(1 << 20, 0xA5, np.uint8))
    ms = C.c_float(float("nan"))
    assert lib.hipk_timer_start(side.ctx) == 0
    assert lib.hipk_memset0(side.ctx, side.ptr(t), 1 << 20) == 0
    assert lib.hipk_timer_stop(side.ctx, C.byref(ms)) == 0
    assert math.isfinite(ms.value) and ms.value >= 0.0


def test_profiler_counts_the_vec_class(side):
    lib = side.lib
    nx = 3
    p = B.Producer(side, B.F32, nx)
    out = side.arr(np.zeros(8))
    ms, launches, nbytes = C.c_double(), C.c_long(), C.c_double()
    get = lambda cls: lib.hipk_prof_get(cls, C.byref(ms), C.byref(launches), C.byref(nbytes))
    try:
        assert lib.hipk_prof_enable(1) == 0 and lib.hipk_prof_reset() == 0
        for _ in range(3):
            p.run(side.ptr(out))
        assert get(B.HIPK_PROF_VEC) == 0
        # hipk_stream_bytes(dt, m, nx) of csrc/hipk_internal.h: m nx elemsize per hipk_col_norms2 call
        assert launches.value == 3 and nbytes.value == 3.0 * B.PROTO_M * nx * 4 and ms.value > 0.0
        assert get(-1) == -1 and get(5) == -1
        assert lib.hipk_prof_reset() == 0
        for cls in range(5):
            assert get(cls) == 0 and (ms.value, launches.value, nbytes.value) == (0.0, 0, 0.0)
        assert lib.hipk_prof_enable(0) == 0
        p.run(side.ptr(out))
        assert get(B.HIPK_PROF_VEC) == 0 and launches.value == 0 and nbytes.value == 0.0
    finally:
        lib.hipk_prof_enable(0)
        lib.hipk_prof_reset()


# ---- D. hipk_sym_eig, hipk_larnv_uniform11 -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", B.EIG_N)
@pytest.mark.parametrize("kind", B.EIG_KINDS)
def test_sym_eig_shapes(side, kind, n):
    B.run_sym_eig(side, kind, n)


def test_sym_eig_declines_65(side):
    A = np.asfortranarray(np.eye(65))
    ev, Z = np.zeros(65), np.zeros((65, 65), order="F")
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert side.lib.hipk_sym_eig(side.ctx, 65, vp(A), 65, vp(ev), vp(Z), 65) == -1
    assert not ev.any() and not Z.any()


@pytest.mark.parametrize("dt", B.TYPES, ids=TID)
@pytest.mark.parametrize("seed", B.LARNV_SEEDS, ids=lambda s: "-".join(map(str, s)))
def test_larnv_seeds_and_sizes(side, dt, seed):
    for n in B.LARNV_N + [0]:
        B.run_larnv(side, dt, seed, n)
    if seed == (1, 3, 5, 7):                                    # not in tests/golden/lapack_dlarnv.json: against the host routine
        x = side.arr(np.zeros(300, B.NPDT[dt]))
        s = (C.c_int64 * 4)(*seed)
        assert side.lib.hipk_larnv_uniform11(side.ctx, dt, s, 300, side.ptr(x)) == 0
        ref, after = B.host_larnv(seed, 300)
        assert np.array_equal(side.get(x), ref.astype(B.NPDT[dt])) and list(s) == after
