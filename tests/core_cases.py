"""Cases, references and the restated host dispatch for the tests of csrc/hipk_core.hip: the second stage of every reduction
(hipk_finalize_kernel in its three layouts), the pinned result mirror with its completion flag and sequence numbers, the
host <-> device copy routing, the small utilities, and two holes of the older tests of this file (hipk_sym_eig,
hipk_larnv_uniform11).  tests/test_core_host.py runs what the plain-C oracle implements and asserts the coverage of the
tables, tests/test_core_gpu.py runs everything on the device through kernel_harness.Dev.

A. Second stage.
  * partial-major, nout = 1: hipk_csr_matvec_scaled on the row tiles launches gx = 8 ceil(ntiles / 8) workgroups whatever the
    device, one partial sum each, so that every (block size, loop region) cell of fin_block_for / hipk_finalize_kernel is reached
    with a two-entries-per-row matrix of n = 256 ntiles - 3 rows (tiles cut at the 256-row limit, the last one ragged).
    fin_regions() restates the kernel's loop: thread t makes a 4-way round while t + 3 nt < nblocks and then adds up to three
    clamped tail terms.  Reference: a = 1 / sqrt(7.5); xout and y are checked element-wise against float64 forms rounded to T,
    the dot is the np.longdouble sum of xout y over the values the device stored, under bound_red(n, sum |xout y|) of
    tests/panel_branch_cases.py with nothing added: a dropped or doubled partial is a relative error of about 1 / gx.
  * o-major (hipk_finalize_partials_t): hipk_panel_project with nrm2_dev, nx in {1, 3}, and hipk_ritz_residual_overlaps.
  * strided with pstride != nout (hipk_finalize_partials_strided(.., nsl, 1, ..) of ritz_ov_t): hipk_ritz_update_overlaps, the
    one entry point that launches it.
    These grids are capped by the CU count; m = 4099 gives at least two partial sums on any device (min_partials restates
    the grid formulas).  The runners, references and bounds are those of tests/panel_branch_cases.py.
B. Mirror, flag, sequence numbers: MirrorRig and the proto_* functions.  The pinned array has 64 spare doubles behind the
   declared mirror so that a store past its end lands in memory the test owns.
C. Copies: copy_route() restates small_copy / pinned_has / foreign_pinned of hipk_h2d / hipk_d2h; COPY_CASES; run_copy.
D. sym_eig_cases / larnv cases.
"""
import ctypes as C
import functools
import math
import os
import time

import numpy as np

from primme_amd import _ffi as F
import checkers
import csr_cases as CC
import panel_branch_cases as P
from panel_branch_cases import bound_red, bound_elem, LD, NPDT, TNAME, F64, F32, Report      # noqa: F401
from csr_branch_cases import bound_row
from reference_kernel_cases import _hu

TYPES = [F64, F32]
BLOCK, FIN_MAXBLOCK = 256, 1024
HIPK_PROF_VEC = 4
_vp, _i = C.c_void_p, C.c_int


def declare(lib):
    """the entry points of this layer that primme_amd/_ffi.py does not declare (and the form switches of the device library)"""
    sig = {"hipk_ctx_set_mirror": ([_vp, _vp, _vp, C.c_size_t], _i), "hipk_wait_results": ([_vp], _i),
           "hipk_wait_seq": ([_vp, C.c_ulonglong], _i), "hipk_seq_issued": ([_vp], C.c_ulonglong),
           "hipk_publish_results": ([_vp, _vp, _i], _i), "hipk_skip_next_flag": ([_vp], None),
           "hipk_d2d": ([_vp, _vp, _vp, C.c_size_t], _i), "hipk_memset0": ([_vp, _vp, C.c_size_t], _i),
           "hipk_is_device_ptr": ([_vp], _i), "hipk_prof_reset": ([], _i), "hipk_prof_enable": ([_i], _i),
           "hipk_set_spmv_format": ([_i], _i), "hipk_csr_format": ([_vp], _i)}
    for name, (args, res) in sig.items():
        if hasattr(lib, name):
            getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    return lib


# What the plain-C oracle cannot tell apart or does not implement, by name and with the reason.  Nothing here is asserted on it.
ORACLE_SAME = {
    "hipk_seq_issued": "always 0: the oracle runs every call to completion, there is no flag to number",
    "hipk_wait_seq / hipk_wait_results": "return 0 and do nothing: results are complete when the producing call returns",
    "hipk_skip_next_flag": "does nothing: there is no flag to skip",
    "hipk_publish_results": "copies into the mirror and returns 0 whatever the range or the context (no bounds, no HIPK_NO_SPINWAIT)",
    "mirror bound": "hipk_cpu_mirror tests the first element only and copies the whole range: the straddling case is device-only",
    "hipk_is_device_ptr": "answers p != NULL: there is one address space",
    "hipk_prof_*": "counters are always 0",
    "copy routing": "every copy is a memmove: library-pinned, caller-pinned and pageable memory take the same path",
    "second stage": "one sequential sum per reduction: no block sizes, no layouts; hipk_set_spmv_format does not exist",
    "hipk_sym_eig n > 64": "the oracle has no size limit (the device kernel holds the matrix in LDS and returns -1)",
}


# ------------------------------------------------------------------------------------------------------------------
# A. the second stage, restated
# ------------------------------------------------------------------------------------------------------------------
def fin_block_for(nblocks):
    """fin_block_for of csrc/hipk_core.hip"""
    return BLOCK if nblocks <= 1024 else 512 if nblocks <= 2048 else FIN_MAXBLOCK


def fin_regions(nblocks):
    """THIS MIRRORS hipk_finalize_kernel: (threads, which threads make a 4-way round: 'none' | 'some' | 'all', the largest
    number of rounds, the set of live tail terms per thread)"""
    nt = fin_block_for(nblocks)
    rounds, live = [], set()
    for t in range(nt):
        r = 0 if nblocks <= t + 3 * nt else -(-(nblocks - t - 3 * nt) // (4 * nt))
        b = t + 4 * nt * r
        rounds.append(r)
        live.add(sum(1 for j in range(3) if b + j * nt < nblocks))
    looped = "none" if max(rounds) == 0 else "all" if min(rounds) > 0 else "some"
    return nt, looped, max(rounds), frozenset(live)


def scaled_gx(ntiles):
    """the grid of hipk_csr_matvec_scaled on the row tiles (csrc/hipk_csr.hip)"""
    return 8 * (-(-ntiles // 8))


# (gx the issue asks for, ntiles that gives it); one ntiles % 8 != 0 per block-size class: its surplus workgroups' partials are summed
SCALED_TILES = [(8, 8), (8, 5), (768, 768), (776, 771), (1024, 1024), (1032, 1032), (1544, 1539), (2048, 2048), (2056, 2056),
                (3080, 3080), (4104, 4099)]
SCALED_CASES = [dict(ep="scaled", dt=dt, gx=gx, ntiles=nt) for dt in TYPES for gx, nt in SCALED_TILES]
NROWS_MAX = 256 * max(nt for _, nt in SCALED_TILES) - 3
NORM2 = 7.5
FIN_M = 4099
OMAJOR_CASES = [dict(ep="project", dt=dt, m=FIN_M, nx=nx, tot=8, split=1, norms=True, place="in", flavour="vec", fin=False, size="l")
                for dt in TYPES for nx in (1, 3)] + \
               [dict(ep="residual", dt=dt, m=FIN_M, k=8, L=3, wtr=1, flavour="vec", size="l") for dt in TYPES]
STRIDED_CASES = [dict(ep="update_overlaps", dt=dt, m=FIN_M, k=8, nb=2, L=3, inplace=False, flavour="vec", size="l") for dt in TYPES]

FIN_CELLS = {(nt, lp) for nt in (256, 512, 1024) for lp in ("none", "some", "all")}
# what no case reaches, with the reason
FIN_UNREACHABLE = {
    ("rounds >= 2", 256): "needs more than 7 * 256 partials, and fin_block_for leaves 256 threads at 1024",
    ("rounds >= 2", 512): "needs more than 7 * 512 partials, and fin_block_for leaves 512 threads at 2048",
    ("rounds >= 2", 1024): "needs more than 7168 partials: a 1.8 M-row matrix, above the 25 MB the largest object of this suite may have",
    ("XR", "any"): "the cross-rank variant runs only when a peer-to-peer communicator armed it (tests/test_multirank_ipc_gpu.py)",
    ("block > 256", "o-major / strided"): "the producers of these layouts cap their grid at 4 (2) workgroups per CU: at most 1024 partials on 256 CUs",
}


def min_partials(c, num_cu=1):
    """the grid (= number of partial sums per output) of the o-major / strided producers, from their launchers' formulas"""
    vw = 16 // np.dtype(NPDT[c["dt"]]).itemsize
    rows = lambda m, per, bpc: max(1, min(-(-m // per), num_cu * bpc))
    if c["ep"] == "project":
        return rows(c["m"] // vw + 1, BLOCK * 2, 4)                   # panel_project_v (flavour 'vec')
    if c["ep"] == "residual":
        return rows(c["m"], 64 * 2, 2)                                # ritz_cgs_t, 16-byte path
    if c["ep"] == "update_overlaps":
        return rows(c["m"], BLOCK * 2, 4)                             # ritz_ov_t
    raise ValueError(c["ep"])


def fin_layout_of(c):
    return {"scaled": "partial-major nout=1", "project": "o-major", "residual": "o-major", "update_overlaps": "strided pstride!=nout"}[c["ep"]]


def case_id(c):
    if c["ep"] == "scaled":
        return f"scaled[{TNAME[c['dt']]},gx={c['gx']},ntiles={c['ntiles']}]"
    return P.case_id(c)


@functools.lru_cache(maxsize=None)
def big_matrix(dt):
    """NROWS_MAX rows, row 0 = {0, 1}, row i = {i - 1, i}: every row prefix of at least two rows is a square matrix"""
    n = NROWS_MAX
    rp = (2 * np.arange(n + 1, dtype=np.int64)).astype(np.int32)
    ci = np.empty(2 * n, np.int32)
    ci[0::2] = np.arange(n) - 1
    ci[1::2] = np.arange(n)
    ci[0], ci[1] = 0, 1
    va = (1.0 + _hu(np.arange(2 * n), 0, 11)).astype(NPDT[dt])          # in [0.5, 1.5): no cancellation that hides a term
    x = _hu(np.arange(n), 0, 21).astype(NPDT[dt])
    for a in (rp, ci, va, x):
        a.setflags(write=False)
    return rp, ci, va, x


def scaled_plan(c):
    rp, ci, va, _ = big_matrix(F64)
    n = 256 * c["ntiles"] - 3
    return CC.tile_plan(checkers.load_hostcheck(), rp[:n + 1], ci[:2 * n], va[:2 * n])


def _run_scaled(side, c, rep):
    dt, cid, npdt = c["dt"], case_id(c), np.dtype(NPDT[c["dt"]])
    n = 256 * c["ntiles"] - 3
    assert scaled_gx(c["ntiles"]) == c["gx"], cid
    plan = scaled_plan(c)
    assert plan.ntiles == c["ntiles"] and plan.tiles[-1] == n and np.all(np.diff(plan.tiles)[:-1] == CC.TILE_ROWS), cid
    rp, ci, va, x = big_matrix(dt)
    rp, ci, va, x = rp[:n + 1], np.ascontiguousarray(ci[:2 * n]), np.ascontiguousarray(va[:2 * n]), x[:n]
    declare(side.lib)
    dev = side.name == "hip" and hasattr(side.lib, "hipk_set_spmv_format")
    old = side.lib.hipk_set_spmv_format(0) if dev else None
    A = C.c_void_p()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    try:
        assert side.lib.hipk_csr_create(side.ctx, dt, n, n, 0, vp(rp), vp(ci), vp(va), C.byref(A)) == 0 and A, cid
        if dev:
            assert side.lib.hipk_csr_format(A) == 0, f"{cid}: not on the row tiles"
        nan3 = np.full(3, np.nan)
        tx, tn = side.arr(x), side.arr(np.array([NORM2, np.nan]))
        txo, ty = side.arr(np.full(n + 2, np.nan, npdt)), side.arr(np.full(n + 2, np.nan, npdt))
        tds = [side.arr(nan3), side.arr(nan3)]
        for td in tds:
            rc = side.lib.hipk_csr_matvec_scaled(A, side.ctx, side.ptr(tx), side.ptr(tn), side.ptr(txo), side.ptr(ty), side.ptr(td))
            assert rc == 0, f"{cid}: rc = {rc}"
        xo, y, d1, d2 = side.get(txo), side.get(ty), side.get(tds[0]), side.get(tds[1])
    finally:
        if A:
            side.lib.hipk_csr_destroy(A)
        if dev:
            side.lib.hipk_set_spmv_format(old)
    rep.same_bits(f"{cid} dot: the same call twice", d1, d2)
    if not (np.isnan(d1[1:]).all() and np.isnan(xo[n:]).all() and np.isnan(y[n:]).all()):
        rep.fails.append(f"{cid}: an element behind an output was written")
    xo, y = xo[:n], y[:n]
    a = 1.0 / math.sqrt(NORM2)
    ax = a * x.astype(np.float64)
    rep.cmp(f"{cid} xout", xo, ax, bound_elem(dt, 1, np.abs(ax)))
    xs = np.asarray(xo, LD)
    t0, t1 = np.asarray(va[0::2], LD) * xs[ci[0::2]], np.asarray(va[1::2], LD) * xs[ci[1::2]]
    rep.cmp(f"{cid} y", y, t0 + t1, bound_row(dt, 2, np.abs(t0) + np.abs(t1)))
    yl = np.asarray(y, LD)
    ref, S = (xs * yl).sum(), (np.abs(xs) * np.abs(yl)).sum()
    bound = bound_red(n, S)
    print(f"{cid}: dot {d1[0]!r}, |error| {float(abs(LD(d1[0]) - ref)):.3g}, bound {float(bound):.3g}, S / gx {float(S) / c['gx']:.3g}")
    assert float(S) / c["gx"] > 100 * float(bound)                 # one partial more or less is far outside the bound
    rep.cmp(f"{cid} dot", d1[0], ref, bound)


RUNNERS = dict(P._RUN, scaled=_run_scaled)


def run_cases(side_factory, cases):
    return P.run_cases(side_factory, cases, RUNNERS)


# ------------------------------------------------------------------------------------------------------------------
# B. mirror, flag and sequence numbers
# ------------------------------------------------------------------------------------------------------------------
SENT_H = np.array([0x7FF8DEAD00000001], np.uint64).view(np.float64)[0]       # two distinct quiet NaNs
SENT_D = np.array([0x7FF8BEEF00000002], np.uint64).view(np.float64)[0]
SPARE = 64
PROTO_M = 4099


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class MirrorRig:
    """a library-pinned host array and a device array of N + 64 doubles, sentinels in both, declared as the mirror of N doubles"""

    def __init__(self, side, N, ctx=None, declare_mirror=True):
        self.side, self.lib, self.N, self.ctx = side, declare(side.lib), N, ctx or side.ctx
        self.hp = C.c_void_p()
        assert self.lib.hipk_host_alloc(self.ctx, (N + SPARE) * 8, C.byref(self.hp)) == 0 and self.hp
        self.h = np.ctypeslib.as_array((C.c_double * (N + SPARE)).from_address(self.hp.value))
        self.h[:] = SENT_H
        self.d = side.arr(np.full(N + SPARE, SENT_D))
        self.written = np.zeros(N + SPARE, bool)
        if declare_mirror:
            assert self.lib.hipk_ctx_set_mirror(self.ctx, side.ptr(self.d), self.hp, N) == 0

    def dptr(self, off):
        return self.side.ptr(self.d, off)

    def seq(self):
        return int(self.lib.hipk_seq_issued(self.ctx))

    def snapshot(self):
        return self.h.copy()

    def untouched(self, what, lo=0, hi=None):
        hi = self.N + SPARE if hi is None else hi
        keep = ~self.written[lo:hi]
        assert np.array_equal(bits(self.h[lo:hi])[keep], np.full(int(keep.sum()), bits(SENT_H)[0])), f"{what}: pinned slots outside the results changed"

    def valid(self, what, off, ref, bound, snap=None):
        """mirror == device bit for bit (the device read back with hipk_d2h), both within the bound, the rest sentinel"""
        n = len(ref)
        self.written[off:off + n] = True
        dev = self.side.get(self.d)
        host = (self.h if snap is None else snap)[off:off + n]
        assert np.array_equal(bits(host), bits(dev[off:off + n])), f"{what}: mirror {host} != device {dev[off:off + n]}"
        err = np.abs(np.asarray(dev[off:off + n], LD) - np.asarray(ref, LD))
        assert np.all(np.isfinite(dev[off:off + n])) and np.all(err <= np.asarray(bound, LD)), f"{what}: error {err} > bound {bound}"
        self.untouched(what)
        keep = ~self.written
        assert np.array_equal(bits(dev)[keep], np.full(int(keep.sum()), bits(SENT_D)[0])), f"{what}: device slots outside the results changed"

    def device_right(self, what, t, off, ref, bound):
        dev = self.side.get(t)[off:off + len(ref)]
        err = np.abs(np.asarray(dev, LD) - np.asarray(ref, LD))
        assert np.all(np.isfinite(dev)) and np.all(err <= np.asarray(bound, LD)), f"{what}: error {err} > bound {bound}"

    def close(self):
        self.lib.hipk_sync(self.ctx)
        self.lib.hipk_ctx_set_mirror(self.ctx, None, None, 0)
        self.lib.hipk_host_free(self.ctx, self.hp)


@functools.lru_cache(maxsize=None)
def norms_input(dt, nx, salt=0):
    """(X (nx, m) in T, sum x^2 in longdouble, bound_red): the producer of the protocol tests"""
    X = (_hu(np.arange(PROTO_M)[None, :], np.arange(nx)[:, None], 41 + salt) * np.linspace(1.0, 3.0, nx)[:, None]).astype(NPDT[dt])
    xl = np.asarray(X, LD)
    ref = (xl * xl).sum(axis=1)
    X.setflags(write=False)
    return X, ref, bound_red(PROTO_M, ref)


class Producer:
    """hipk_col_norms2 of an uploaded m = 4099 panel into any device address"""

    def __init__(self, side, dt, nx, salt=0, ctx=None):
        self.side, self.dt, self.nx, self.ctx = side, dt, nx, ctx or side.ctx
        X, self.ref, self.bound = norms_input(dt, nx, salt)
        self.t = side.arr(X)

    def run(self, out_ptr):
        rc = self.side.lib.hipk_col_norms2(self.ctx, self.dt, PROTO_M, self.side.ptr(self.t), PROTO_M, self.nx, out_ptr)
        assert rc == 0, rc


def proto_flagged(side, dt, nx, off, N=40):
    """B1; on the oracle (no flag) the mirror contents alone"""
    rig, dev = MirrorRig(side, N), side.name == "hip"
    try:
        p = Producer(side, dt, nx)
        s0 = rig.seq()
        p.run(rig.dptr(off))
        if dev:
            assert rig.seq() == s0 + 1
        assert rig.lib.hipk_wait_results(rig.ctx) == 0
        snap = rig.snapshot()
        rig.valid(f"flagged off={off}", off, p.ref, p.bound, snap)
    finally:
        rig.close()


def proto_unmirrored(side, dt, nx, where, N=40):
    """B2: a separate buffer, or one past the end of the mirror"""
    rig = MirrorRig(side, N)
    try:
        p = Producer(side, dt, nx)
        other = side.arr(np.full(8, SENT_D))
        t, off = (other, 0) if where == "separate" else (rig.d, N)
        s0 = rig.seq()
        p.run(side.ptr(t, off))
        assert rig.seq() == s0
        assert rig.lib.hipk_wait_results(rig.ctx) == 0
        rig.untouched(f"unmirrored {where}")                     # before any other synchronisation: the wait drained
        rig.device_right(f"unmirrored {where}", t, off, p.ref, p.bound)
    finally:
        rig.close()


def proto_straddle(side, dt, N=40):
    """B3: three results at d + N - 1: the first inside the declared mirror, two past its end"""
    rig = MirrorRig(side, N)
    try:
        p = Producer(side, dt, 3)
        s0 = rig.seq()
        p.run(rig.dptr(N - 1))
        s1 = rig.seq()
        assert rig.lib.hipk_wait_results(rig.ctx) == 0
        rig.device_right("straddle", rig.d, N - 1, p.ref, p.bound)
        print(f"straddle: h[N-1 .. N+2) = {bits(rig.h[N - 1:N + 2])}, seq {s0} -> {s1}")
        rig.untouched("straddle: stores past the declared end of the mirror", N, N + SPARE)
        assert s1 == s0, "a range that is not wholly inside the mirror is not mirrored: no flag"
        rig.untouched("straddle: no host store at all")
    finally:
        rig.close()


def proto_wait_seq(side, dt, N=40):
    """B4"""
    rig = MirrorRig(side, N)
    try:
        ps = [Producer(side, dt, 3, salt=s) for s in range(3)]
        offs, seqs = [0, 5, 10], []
        for p, off in zip(ps, offs):
            p.run(rig.dptr(off))
            seqs.append(rig.seq())
        assert seqs[1] == seqs[0] + 1 and seqs[2] == seqs[1] + 1
        assert rig.lib.hipk_wait_seq(rig.ctx, seqs[0]) == 0
        snap_a = rig.snapshot()
        assert rig.lib.hipk_wait_seq(rig.ctx, seqs[2]) == 0
        snap = rig.snapshot()
        assert rig.lib.hipk_wait_seq(rig.ctx, 0) == 0 and rig.lib.hipk_wait_seq(rig.ctx, seqs[2] + 5) == 0       # the drain path
        assert rig.lib.hipk_wait_results(rig.ctx) == 0 and rig.seq() == seqs[2]
        for p, off in zip(ps, offs):
            rig.written[off:off + 3] = True
        rig.valid("wait_seq(s1): A", offs[0], ps[0].ref, ps[0].bound, snap_a)
        for p, off, nm in zip(ps, offs, "ABC"):
            rig.valid(f"wait_seq(s3): {nm}", off, p.ref, p.bound, snap)
    finally:
        rig.close()


def proto_skip(side, dt, N=40):
    """B5"""
    rig = MirrorRig(side, N)
    try:
        ps = [Producer(side, dt, 3, salt=s) for s in range(4)]
        s0 = rig.seq()
        rig.lib.hipk_skip_next_flag(rig.ctx)
        ps[0].run(rig.dptr(0))
        assert rig.seq() == s0
        ps[1].run(rig.dptr(5))
        assert rig.seq() == s0 + 1
        assert rig.lib.hipk_wait_results(rig.ctx) == 0
        snap = rig.snapshot()
        rig.written[0:3] = rig.written[5:8] = True
        rig.valid("skip: the unflagged first", 0, ps[0].ref, ps[0].bound, snap)
        rig.valid("skip: the flagged second", 5, ps[1].ref, ps[1].bound, snap)
        ps[2].run(rig.dptr(10))
        assert rig.seq() == s0 + 2                               # one-shot
        assert rig.lib.hipk_wait_results(rig.ctx) == 0
        rig.valid("skip: the third", 10, ps[2].ref, ps[2].bound, rig.snapshot())
        rig.lib.hipk_skip_next_flag(rig.ctx)
        ps[3].run(rig.dptr(15))
        assert rig.seq() == s0 + 2
        assert rig.lib.hipk_wait_results(rig.ctx) == 0           # nothing flagged after the skipped one: drains
        rig.valid("skip, then wait", 15, ps[3].ref, ps[3].bound, rig.snapshot())
    finally:
        rig.close()


PUBLISH_COUNTS = [1, 256, 257, 1000]


def proto_publish(side, count, N=1024, off=3):
    """B6, the accepted ranges; on the oracle the mirror contents alone"""
    rig, dev = MirrorRig(side, N), side.name == "hip"
    try:
        vals = np.ascontiguousarray(_hu(np.arange(count), 0, 31))
        assert rig.lib.hipk_h2d(rig.ctx, rig.dptr(off), vals.ctypes.data_as(C.c_void_p), count * 8) == 0
        s0 = rig.seq()
        assert rig.lib.hipk_publish_results(rig.ctx, rig.dptr(off), count) == 0
        if dev:
            assert rig.seq() == s0 + 1
        assert rig.lib.hipk_wait_results(rig.ctx) == 0
        assert np.array_equal(bits(rig.h[off:off + count]), bits(vals))
        rig.written[off:off + count] = True
        rig.untouched(f"publish {count}")
        for cnt in ((0, -3) if dev else (0,)):                      # count <= 0: nothing is enqueued
            assert rig.lib.hipk_publish_results(rig.ctx, rig.dptr(off), cnt) == 0 and rig.seq() == s0 + (1 if dev else 0)
        if dev:
            assert rig.lib.hipk_wait_results(rig.ctx) == 0
            rig.untouched(f"publish {count}, then count <= 0")
    finally:
        rig.close()


def proto_publish_declined(side, N=1024):
    """B6, the three refusals: 1, no sequence number, mirror untouched"""
    rig = MirrorRig(side, N)
    try:
        s0 = rig.seq()
        assert rig.lib.hipk_publish_results(rig.ctx, rig.dptr(N), 4) == 1                    # the start outside
        assert rig.lib.hipk_publish_results(rig.ctx, rig.dptr(N - 2), 5) == 1                # the end outside
        other = side.arr(np.zeros(8))
        assert rig.lib.hipk_publish_results(rig.ctx, side.ptr(other), 4) == 1
        assert rig.seq() == s0 and rig.lib.hipk_sync(rig.ctx) == 0
        rig.untouched("publish declined")
        ctx2 = C.c_void_p()
        os.environ["HIPK_NO_SPINWAIT"] = "1"
        try:
            assert rig.lib.hipk_ctx_create(C.byref(ctx2), None) == 0
        finally:
            del os.environ["HIPK_NO_SPINWAIT"]
        try:
            assert rig.lib.hipk_ctx_set_mirror(ctx2, rig.dptr(0), rig.hp, N) == 0
            q0 = int(rig.lib.hipk_seq_issued(ctx2))
            assert rig.lib.hipk_publish_results(ctx2, rig.dptr(3), 4) == 1
            assert int(rig.lib.hipk_seq_issued(ctx2)) == q0 and rig.lib.hipk_sync(ctx2) == 0
            rig.untouched("publish without spin wait")
        finally:
            rig.lib.hipk_ctx_destroy(ctx2)
    finally:
        rig.close()


TICKET_NOUTS = [1, 5, 64, 1]


def proto_tickets(side, dt, N=128):
    """B7: second stages of 1, 5, 64, 1 blocks in a row; returns the longest wait in seconds (printed, not asserted)"""
    rig = MirrorRig(side, N)
    worst = 0.0
    try:
        off = 0
        for i, nout in enumerate(TICKET_NOUTS):
            s0 = rig.seq()
            if nout == 5:                                            # hipk_panel_dots: 5 basis columns against one vector
                A = (_hu(np.arange(PROTO_M)[None, :], np.arange(5)[:, None], 51) * np.linspace(0.5, 2.0, 5)[:, None]).astype(NPDT[dt])
                x = _hu(np.arange(PROTO_M), 0, 52).astype(NPDT[dt])
                ta, tx = side.arr(A), side.arr(x)
                seg = (F.HipkSeg * 1)()
                seg[0].base, seg[0].ld, seg[0].ncols = side.ptr(ta).value, PROTO_M, 5
                assert side.lib.hipk_panel_dots(rig.ctx, dt, PROTO_M, seg, 1, side.ptr(tx), PROTO_M, 1, rig.dptr(off), 5) == 0
                r, S = P.ref_dots(A, x[None, :])
                ref, bound = r[0], bound_red(PROTO_M, S[0])
            else:
                p = Producer(side, dt, nout, salt=10 + i)
                p.run(rig.dptr(off))
                ref, bound = p.ref, p.bound
            assert rig.seq() == s0 + 1, f"nout = {nout}"
            t0 = time.perf_counter()
            assert rig.lib.hipk_wait_results(rig.ctx) == 0
            worst = max(worst, time.perf_counter() - t0)
            rig.valid(f"tickets nout={nout}", off, ref, bound, rig.snapshot())
            off += nout + 3
    finally:
        rig.close()
    return worst


def proto_mirror_off(side, dt, N=40):
    """B8"""
    rig = MirrorRig(side, N)
    try:
        assert rig.lib.hipk_ctx_set_mirror(rig.ctx, None, None, 0) == 0
        p = Producer(side, dt, 3)
        s0 = rig.seq()
        p.run(rig.dptr(0))
        assert rig.seq() == s0 and rig.lib.hipk_wait_results(rig.ctx) == 0
        rig.untouched("mirror off")
        rig.device_right("mirror off", rig.d, 0, p.ref, p.bound)
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------------
# C. copies
# ------------------------------------------------------------------------------------------------------------------
COPY_KERNEL_MAX, STAGE_MIN, STAGE_MAX = 1 << 20, 1 << 16, 32 << 20
PAD = 64                                                    # sentinel bytes on both sides of every destination


def ramp(n, salt=0):
    return ((np.arange(n, dtype=np.int64) * 131 + 7 + salt) & 0xFF).astype(np.uint8)


def copy_route(kind, nbytes, host_off=0, dev_off=0, stage_cap=0):
    """THIS MIRRORS hipk_h2d / hipk_d2h of csrc/hipk_core.hip (pinned_has, foreign_pinned, small_copy, ctx_stage): the path
    a copy takes, as a tuple.  kind: 'lib' (hipk_host_alloc), 'foreign' (pinned by the caller), 'pageable'.  Library and
    device allocations are at least 256-byte aligned, so the offsets decide the alignment."""
    if nbytes == 0:
        return ("nothing",)
    if kind == "pageable":
        want = min(nbytes, STAGE_MAX)
        cap, grown = stage_cap, False
        if want > cap:
            cap, grown = STAGE_MIN, True
            while cap < want:
                cap *= 2
        chunks = -(-nbytes // cap)
        return ("staged", "grow" if grown else "reuse", "one chunk" if chunks == 1 else "chunks, ragged last" if nbytes % cap else "chunks")
    if kind == "foreign":
        return ("runtime", "foreign")
    assert kind == "lib"
    if nbytes > COPY_KERNEL_MAX:
        return ("runtime", "lib: over 1 MiB")
    if nbytes & 3:
        return ("runtime", "lib: bytes % 4")
    if host_off & 3:
        return ("runtime", "lib: pinned side unaligned")
    if dev_off & 3:
        return ("runtime", "lib: device side unaligned")
    nw = nbytes // 4
    gx = min(-(-nw // BLOCK), 64)
    return ("copy kernel", "grid-stride" if nw > gx * BLOCK else "one pass", "full blocks" if nw % BLOCK == 0 else "ragged block")


def _copy_cases():
    out = []
    for n in (4, 8, 1020, 65536, 65540, 1048576):
        out += [dict(kind="lib", n=n, host_off=h, dev_off=d) for h, d in ((0, 0), (4, 0), (0, 4))]
    out += [dict(kind="lib", n=6, host_off=0, dev_off=0), dict(kind="lib", n=1048580, host_off=0, dev_off=0),
            dict(kind="lib", n=1024, host_off=2, dev_off=0), dict(kind="lib", n=1024, host_off=0, dev_off=2)]
    out += [dict(kind="foreign", n=n, host_off=0, dev_off=0) for n in (1024, 2000000)]
    # in this order on one fresh context: the staging buffer grows at 1 (64 KB), 65 537 (128 KB) and at the two-chunk copy
    out += [dict(kind="pageable", n=n, host_off=1, dev_off=3) for n in (1, 7, 65537, (32 << 20) + 4099, 100)]
    out += [dict(kind=k, n=0, host_off=0, dev_off=0) for k in ("lib", "pageable")]
    return out


COPY_CASES = _copy_cases()
COPY_ROUTES_WANTED = ({("nothing",), ("runtime", "foreign"), ("runtime", "lib: over 1 MiB"), ("runtime", "lib: bytes % 4"),
                       ("runtime", "lib: pinned side unaligned"), ("runtime", "lib: device side unaligned"),
                       ("copy kernel", "one pass", "full blocks"), ("copy kernel", "one pass", "ragged block"),
                       ("copy kernel", "grid-stride", "full blocks"), ("copy kernel", "grid-stride", "ragged block"),
                       ("staged", "grow", "one chunk"), ("staged", "reuse", "one chunk"), ("staged", "grow", "chunks, ragged last")})
COPY_UNREACHABLE = {
    ("HIPK_NO_COPY_KERNEL",): "read once per process, and no test of this suite may start a child process or keep a HIPK_* variable set",
    ("more than 256 pinned buffers",): "pinned_note's overflow path needs 257 live hipk_host_alloc buffers; it only prints and takes the runtime path",
    ("staged", "chunks"): "whole chunks only would need a multiple of 32 MB: the ragged two-chunk copy runs the same loop",
    ("staged", "reuse", "chunks, ragged last"): "a second copy above 32 MB, which the size limit of this suite leaves out",
}


def copy_routes(cases):
    """the route of every case, the pageable ones with the staging capacity the earlier ones of the list left"""
    cap, out = 0, []
    for c in cases:
        r = copy_route(c["kind"], c["n"], c["host_off"], c["dev_off"], cap)
        if c["kind"] == "pageable" and c["n"]:
            want = min(c["n"], STAGE_MAX)
            if want > cap:
                cap = STAGE_MIN
                while cap < want:
                    cap *= 2
        out.append(r)
    return out


def copy_id(c):
    return f"{c['kind']}-{c['n']}-h{c['host_off']}-d{c['dev_off']}"


class CopyRig:
    """one context's buffers for the copy cases: a device buffer, a library-pinned one, and the caller's own"""

    def __init__(self, side, cap):
        # an odd number of bytes: the whole-buffer copies that fill and read the device side for the comparison then take the
        # runtime's path whatever the size, never the copy kernel under test
        self.side, self.lib, self.cap = side, declare(side.lib), (cap + 2 * PAD + 8) // 4 * 4 + 5
        self.dev = C.c_void_p()
        assert self.lib.hipk_malloc(side.ctx, self.cap, C.byref(self.dev)) == 0
        self.pin = C.c_void_p()
        assert self.lib.hipk_host_alloc(side.ctx, self.cap, C.byref(self.pin)) == 0
        self.pinv = np.ctypeslib.as_array((C.c_uint8 * self.cap).from_address(self.pin.value))
        self.check = C.c_void_p()                                   # read-back path of its own: pinned, runtime-sized or kernel-sized alike
        assert self.lib.hipk_host_alloc(side.ctx, self.cap, C.byref(self.check)) == 0
        self.checkv = np.ctypeslib.as_array((C.c_uint8 * self.cap).from_address(self.check.value))

    def dev_fill(self, byte):
        """the whole device buffer = `byte`, through a pinned upload on the runtime's path"""
        self.checkv[:] = byte
        assert self.lib.hipk_h2d(self.side.ctx, self.dev, self.check, self.cap) == 0 and self.lib.hipk_sync(self.side.ctx) == 0

    def dev_read(self):
        self.checkv[:] = 0x3C
        assert self.lib.hipk_d2h(self.side.ctx, self.check, self.dev, self.cap) == 0 and self.lib.hipk_sync(self.side.ctx) == 0
        return self.checkv.copy()

    def close(self):
        self.lib.hipk_sync(self.side.ctx)
        self.lib.hipk_free(self.side.ctx, self.dev)
        self.lib.hipk_host_free(self.side.ctx, self.pin)
        self.lib.hipk_host_free(self.side.ctx, self.check)


def run_copy(side, rig, c, foreign=None):
    """one case in both directions, byte for byte, sentinels on both sides of the destination.  foreign: a uint8 numpy view of
    the caller's own pinned memory (kind 'foreign')"""
    lib, ctx, n, ho, do = rig.lib, side.ctx, c["n"], c["host_off"], c["dev_off"]
    cid = copy_id(c)
    assert PAD + max(ho, do) + n + PAD <= rig.cap, f"{cid}: the rig's buffers are too small for this case"
    src = ramp(n)
    dptr = C.c_void_p(rig.dev.value + PAD + do)
    if c["kind"] == "lib":
        hview, hbase = rig.pinv, rig.pin.value
    elif c["kind"] == "foreign":
        hview, hbase = foreign, foreign.ctypes.data
        assert len(foreign) >= PAD + ho + n + PAD
    else:
        hview = np.empty(PAD + ho + n + PAD, np.uint8)
        hbase = hview.ctypes.data
    hptr = C.c_void_p(hbase + PAD + ho)
    # host -> device
    rig.dev_fill(0xA5)
    hview[:] = 0x5A
    hview[PAD + ho:PAD + ho + n] = src
    assert lib.hipk_h2d(ctx, dptr if n else None, hptr if n else None, n) == 0, cid
    if c["kind"] == "pageable":
        hview[PAD + ho:PAD + ho + n] = 0xEE                           # complete on return: the source may change at once
    else:
        assert lib.hipk_sync(ctx) == 0
    got = rig.dev_read()
    want = np.full(rig.cap, 0xA5, np.uint8)
    want[PAD + do:PAD + do + n] = src
    assert np.array_equal(got, want), f"{cid} h2d: first difference at byte {int(np.flatnonzero(got != want)[0]) - PAD - do} of {n}"
    # device -> host
    src2 = ramp(n, salt=91)
    rig.checkv[:] = 0xA5
    rig.checkv[PAD + do:PAD + do + n] = src2
    assert lib.hipk_h2d(ctx, rig.dev, rig.check, rig.cap) == 0 and lib.hipk_sync(ctx) == 0
    hview[:] = 0x5A
    assert lib.hipk_d2h(ctx, hptr if n else None, dptr if n else None, n) == 0, cid
    if c["kind"] != "pageable":
        assert lib.hipk_sync(ctx) == 0                               # the pageable path is complete on return: compared without
    wanth = np.full(len(hview), 0x5A, np.uint8)
    wanth[PAD + ho:PAD + ho + n] = src2
    assert np.array_equal(hview, wanth), f"{cid} d2h: first difference at byte {int(np.flatnonzero(hview != wanth)[0]) - PAD - ho} of {n}"


UTIL_SIZES = [0, 1, 4099, 1 << 20]


def run_d2d(side, n):
    """non-overlapping ranges of one allocation, odd offsets"""
    lib = declare(side.lib)
    a, b = 3, 3 + n + 7 + (n + 7) % 2                                 # both odd
    total = b + n + 5
    buf = np.full(total, 0xA5, np.uint8)
    buf[a:a + n] = ramp(n)
    t = side.arr(buf)
    assert lib.hipk_d2d(side.ctx, side.ptr(t, b), side.ptr(t, a), n) == 0
    want = buf.copy()
    want[b:b + n] = ramp(n)
    assert a % 2 == 1 and b % 2 == 1 and np.array_equal(side.get(t), want)


def run_memset0(side, n):
    lib = declare(side.lib)
    buf = np.full(n + 64, 0xA5, np.uint8)
    t = side.arr(buf)
    assert lib.hipk_memset0(side.ctx, side.ptr(t, 13), n) == 0
    want = buf.copy()
    want[13:13 + n] = 0
    assert np.array_equal(side.get(t), want)


# ------------------------------------------------------------------------------------------------------------------
# D. hipk_sym_eig and hipk_larnv_uniform11
# ------------------------------------------------------------------------------------------------------------------
EIG_N = [2, 15, 16, 64]
EIG_KINDS = ["random", "repeated", "descending diagonal", "zero", "graded"]


def sym_eig_matrix(kind, n):
    rng = np.random.default_rng(1000 + n)
    if kind == "random":
        B = rng.standard_normal((n, n))
        return B + B.T
    if kind == "repeated":
        Q = np.linalg.qr(rng.standard_normal((n, n)))[0]
        d = np.concatenate([np.ones(3), 2.0 + np.arange(max(n - 3, 0))])[:n]
        A = Q @ np.diag(d) @ Q.T
        return 0.5 * (A + A.T)
    if kind == "descending diagonal":
        return np.diag(np.arange(n, 0, -1) * 1.5)
    if kind == "zero":
        return np.zeros((n, n))
    if kind == "graded":
        E = rng.standard_normal((n, n))
        return np.diag(10.0 ** -np.arange(n, dtype=np.float64)) + 1e-12 * (E + E.T)
    raise ValueError(kind)


def run_sym_eig(side, kind, n):
    """lda = ldz = n + 3, NaN in the strictly lower triangle and in the padding rows of A, sentinel rows in Z; the checks of
    tests/test_kernels_gpu.py: test_device_rayleigh_ritz_kernel"""
    A = sym_eig_matrix(kind, n)
    ld = n + 3
    Af = np.full((ld, n), np.nan, order="F")
    Af[:n, :] = np.triu(A)
    Af[:n, :][np.tril_indices(n, -1)] = np.nan
    ev = np.full(n + 1, SENT_H)
    Z = np.full((ld, n), SENT_H, order="F")
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert side.lib.hipk_sym_eig(side.ctx, n, vp(Af), ld, vp(ev), vp(Z), ld) == 0
    assert bits(ev[n:])[0] == bits(SENT_H)[0] and np.all(bits(Z[n:, :]) == bits(SENT_H)[0]), "padding rows of Z / the slot behind evals changed"
    ev, Z = ev[:n], Z[:n, :]
    w = np.linalg.eigvalsh(A)
    scale = max(1.0, np.abs(w).max())
    assert np.all(np.isfinite(ev)) and np.all(np.isfinite(Z))
    assert np.all(np.diff(ev) >= 0), "ascending order"
    assert np.max(np.abs(ev - w)) <= 1e-13 * n * scale
    assert np.linalg.norm(Z.T @ Z - np.eye(n)) <= 1e-13 * n
    assert np.linalg.norm(A @ Z - Z * ev) <= 1e-12 * scale * n


LARNV_SEEDS = [(4095, 4095, 4095, 4095), (0, 0, 0, 1), (1, 3, 5, 7)]
LARNV_N = [256, 257, 512, 513]


def host_larnv(seed, n):
    """pa_larnv_uniform11 of the host solver (checked against LAPACK's DLARNV by tests/test_dense_host.py): (numbers, seed after)"""
    lib = C.CDLL(checkers.HOSTCHECK_LIB)
    s = (C.c_int64 * 4)(*seed)
    x = np.zeros(max(n, 1))
    lib.pa_larnv_uniform11(s, C.c_int64(n), x.ctypes.data_as(C.c_void_p))
    return x[:n], list(s)


def run_larnv(side, dt, seed, n):
    npdt = NPDT[dt]
    sent = npdt(-7.25)
    x = side.arr(np.full(n + 3, sent, npdt))
    s = (C.c_int64 * 4)(*seed)
    assert side.lib.hipk_larnv_uniform11(side.ctx, dt, s, n, side.ptr(x)) == 0
    got = side.get(x)
    assert np.all(got[n:] == sent), "the element behind x[n - 1] changed"
    if n == 0:
        assert list(s) == list(seed)
        return
    ref, after = host_larnv(seed, n)
    assert np.array_equal(got[:n], ref.astype(npdt)) and list(s) == after and list(s) != list(seed)
