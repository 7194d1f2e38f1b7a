"""The Chebyshev polynomial preconditioner of the singular value solver on the MI355X: primme_amd_svds_chebyshev_precond against
the numpy restatement (tests/svds_cheb_cases.py) mode by mode, the one-pass steps against the generic pair, the solver with
precond=("chebyshev", ...) against the checker library with the numpy callback on every case of the table, what the
preconditioner buys on the difference matrix, and the argument checks of primme_amd_svds_operator_set_chebyshev."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import svds_cheb_cases as SC
from primme_amd import _ffi as F
from primme_amd.svds_api import complex_csr_to_real
from test_svds_host import _rect, _rect_complex

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY_LOG = os.path.join(ROOT, "profiles", "svds_cheb_kernel_accuracy.txt")
GOLD = json.load(open(SC.GOLDEN))
MODES = {SC.MODE_ATA: "AtA", SC.MODE_AAT: "AAt", SC.MODE_AUG: "augmented"}
# PRIMME_AMD_CHEB_FUSED=1 (read when the preconditioner is configured): the one-pass step at every width; test_callback_sweep_with_
# the_one_pass_step runs the callback sweep of this module once more in a child process under it
ONE_PASS = os.environ.get("PRIMME_AMD_CHEB_FUSED") == "1" and os.environ.get("PRIMME_AMD_CHEB_UNFUSED", "0") == "0"


@pytest.fixture(scope="module")
def accuracy_log():
    """The callback cases add their figures; a run of the whole sweep rewrites profiles/svds_cheb_kernel_accuracy.txt."""
    lines = []
    yield lines
    if len(lines) >= 27 * len(SWEEPS) and not ONE_PASS:              # the record is that of the default path
        with open(ACCURACY_LOG, "w") as f:
            f.write("primme_amd_svds_chebyshev_precond against the numpy restatement, relative infinity norm; E = distance of the\n"
                    "restatement from the spectral value on the same input; bound = max(8 E, 64 steps u_T)\n")
            f.write("\n".join(lines) + "\n")


def _u(dtype):
    return 2.0 ** -53 if np.dtype(dtype) in (np.dtype(np.float64), np.dtype(np.complex128)) else 2.0 ** -24


class _Operator:
    """A singular value operator of the product library on a context of its own"""

    def __init__(self, m, n, csr, dtype):
        self.lib = lib = F.load_product()
        dtype = np.dtype(dtype)
        self.cplx = dtype.kind == "c"
        rdtype = np.float64 if dtype in (np.dtype(np.float64), np.dtype(np.complex128)) else np.float32
        rp, ci, va = csr
        rp, ci, va = np.ascontiguousarray(rp, dtype=np.int32), np.ascontiguousarray(ci, dtype=np.int32), np.ascontiguousarray(va, dtype=dtype)
        if self.cplx:
            rp, ci, va = complex_csr_to_real(m, rp, ci, va, rdtype)
            m, n = 2 * m, 2 * n
        self.ctx, self.op = C.c_void_p(), C.c_void_p()
        assert lib.hipk_ctx_create(C.byref(self.ctx), None) == 0
        assert lib.primme_amd_svds_operator_create(C.byref(self.op), self.ctx, F.HIPK_F64 if rdtype == np.float64 else F.HIPK_F32, m, n,
                                                   rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p), va.ctypes.data_as(C.c_void_p)) == 0
        if self.cplx:
            assert lib.primme_amd_svds_operator_set_complex(self.op, 1) == 0

    def apply(self, X, mode, ldx, ldy):
        """y = K^-1 x through the callback on device panels; X: (len, nb) in the operator's precision"""
        import torch
        ln, nb = X.shape
        tdt = getattr(torch, str(X.dtype))
        xt = torch.full((nb, ldx), float("nan"), dtype=tdt, device="cuda")
        yt = torch.full((nb, ldy), float("nan"), dtype=tdt, device="cuda")
        xt[:, :ln] = torch.from_numpy(np.ascontiguousarray(X.T)).to("cuda")
        torch.cuda.synchronize()
        ps = F.PrimmeSvdsParams()
        self.lib.primme_svds_initialize(C.byref(ps))
        ps.preconditioner = self.op
        lx, ly, bs, md, ierr = F.PRIMME_INT(ldx), F.PRIMME_INT(ldy), C.c_int(nb), C.c_int(mode), C.c_int(-7)
        self.lib.primme_amd_svds_chebyshev_precond(C.c_void_p(xt.data_ptr()), C.byref(lx), C.c_void_p(yt.data_ptr()), C.byref(ly), C.byref(bs),
                                                   C.byref(md), C.byref(ps), C.byref(ierr))
        assert self.lib.hipk_sync(self.ctx) == 0
        torch.cuda.synchronize()
        y = yt.cpu().numpy()
        assert np.all(np.isnan(y[:, ln:]))                    # padding untouched
        assert np.array_equal(xt.cpu().numpy()[:, :ln], X.T)
        return ierr.value, y[:, :ln].T

    def close(self):
        self.lib.primme_amd_svds_operator_destroy(self.op)
        self.lib.hipk_ctx_destroy(self.ctx)


def _callback_case(accuracy_log, label, m, n, csr, A, dtype, slo, shi, sshift, modes):
    op = _Operator(m, n, csr, dtype)
    wide = np.complex128 if np.dtype(dtype).kind == "c" else np.float64
    Aw = A.astype(dtype).astype(wide)                     # the matrix the device sees
    av, atv = (lambda v: Aw @ v), (lambda u: Aw.conj().T @ u)
    length = {SC.MODE_ATA: n, SC.MODE_AAT: m, SC.MODE_AUG: m + n}
    rng = np.random.default_rng(17)
    try:
        lib = op.lib
        for steps in (1, 2, 8):
            assert lib.primme_amd_svds_operator_set_chebyshev(op.op, steps, slo, shi, sshift) == 0
            for mode in modes:
                ln = length[mode]
                for nb in (1, 3, 9):                      # 9: two chunks
                    X = rng.standard_normal((ln, nb))
                    if wide == np.complex128:
                        X = X + 1j * rng.standard_normal((ln, nb))
                    X = X.astype(dtype)
                    Xw = X.astype(wide)
                    lib.primme_amd_chebyshev_stats(None, None, None)
                    ierr, got = op.apply(X, mode, ln + 3, ln + 8)
                    assert ierr == 0
                    st = [C.c_long() for _ in range(3)]
                    lib.primme_amd_chebyshev_stats(*[C.byref(v) for v in st])
                    per = 2 * (steps - 1) if mode != SC.MODE_AUG else 4 * (steps - 1) + 2
                    assert (st[0].value, st[1].value) == (nb, per * nb)
                    # every product with the second factor is a one-pass step, or none is (the default: profiles/svds_cheb_step_kernels.md)
                    one_pass = (steps - 1 if mode != SC.MODE_AUG else 2 * (steps - 1) + 2) * nb
                    assert st[2].value == (one_pass if ONE_PASS else 0)
                    want = SC.svds_cheb_apply(av, atv, n, Xw, mode, steps, slo, shi, sshift)
                    E = SC.CC.rel_inf(want, SC.svds_cheb_spectral(Aw, Xw, mode, steps, slo, shi, sshift))
                    D = SC.CC.rel_inf(got.astype(wide), want)
                    bound = max(8 * E, 64 * steps * _u(dtype))
                    line = (f"{label:22s} {MODES[mode]:9s} steps={steps} nb={nb}  E(restatement)={E:.3e}  device distance={D:.3e}  "
                            f"bound={bound:.3e}  fused steps={st[2].value}")
                    print(line)
                    accuracy_log.append(line)
                    assert D <= bound, line
        ierr, _ = op.apply(np.zeros((n, 1), dtype=dtype), 0, n + 3, n + 8)        # primme_svds_op_none
        assert ierr == 1
    finally:
        op.close()


ALL_MODES = (SC.MODE_ATA, SC.MODE_AAT, SC.MODE_AUG)
SWEEPS = [("rect300x200", "float64"), ("rect300x200", "float32"), ("D200", "float64"), ("D200", "float32"), ("z_rect120x80", "complex128")]


def _sweep_args(matrix, dtype):
    """label, m, n, csr, dense matrix, dtype, slo, shi, sshift, modes of one callback sweep"""
    dtype = np.dtype(dtype)
    if matrix == "D200":
        m, n, csr = SC.difference_matrix(200)
        return f"{matrix} {dtype.name}", m, n, csr, SC.dense_of(m, n, csr), dtype, 0.055, 2.0, 0.0, ALL_MODES
    (m, n), make = ((300, 200), _rect) if matrix == "rect300x200" else ((120, 80), _rect_complex)
    A, csr = make(m, n)
    s = np.linalg.svd(A, compute_uv=False)
    label = f"{matrix} {dtype.name}" if dtype.kind != "c" else f"{matrix} real-eq."
    return label, m, n, csr, A, dtype, 0.0, float(0.5 * (s[3] + s[4])), SC.norm_bound_numpy(m, n, *csr), ALL_MODES


@pytest.mark.parametrize("matrix,dtype", SWEEPS[:4])
def test_callback_against_the_restatement(built, accuracy_log, matrix, dtype):
    _callback_case(accuracy_log, *_sweep_args(matrix, dtype))


def test_callback_on_the_complex_real_equivalent_form(built, accuracy_log):
    _callback_case(accuracy_log, *_sweep_args(*SWEEPS[4]))


_SWEEP_CHILD = r"""
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/oracle"); sys.path.insert(0, {root!r} + "/tests")
import test_svds_cheb_gpu as T
assert T.ONE_PASS
lines = []
for matrix, dtype in T.SWEEPS:
    T._callback_case(lines, *T._sweep_args(matrix, dtype))
print("RESULT", len(lines), sum("fused steps=0" in ln for ln in lines))
"""


def test_callback_sweep_with_the_one_pass_step(built):
    """Every sweep above once more with PRIMME_AMD_CHEB_FUSED=1, in a child process (the knob is read when the preconditioner is
    configured): every mode, the complex form included, through hipk_csr_cheb_step_gather.  _callback_case asserts the
    fused-step count of the path it runs on; only the steps = 1 lines have no product, hence no fused step."""
    env = dict(os.environ, PRIMME_AMD_CHEB_FUSED="1", PRIMME_AMD_CHEB_UNFUSED="0")
    r = subprocess.run([sys.executable, "-c", _SWEEP_CHILD.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    done, without = (int(v) for v in [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1].split()[1:])
    assert done == 27 * len(SWEEPS) and without == 6 * len(SWEEPS)      # steps = 1 in the two normal-equation modes, 3 widths


_CHILD = r"""
import json, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/oracle"); sys.path.insert(0, {root!r} + "/tests")
import numpy as np
import svds_cheb_cases as SC
out = {{}}
for name in ("D200_s8", "rect200x300"):
    r = SC.run_case(name, "hip")
    out[name] = dict(ret=r.ret, svals=np.asarray(r.svals).tolist(), its=r.stats["numOuterIterations"], stats=r.precond_stats)
print("RESULT " + json.dumps(out))
"""


def _child(env_extra):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def test_fused_against_generic(built):
    """The same solves with the one-pass steps at every width (PRIMME_AMD_CHEB_FUSED=1) and with the generic pair
    (PRIMME_AMD_CHEB_UNFUSED=1), each in a fresh process: the knobs are read when the preconditioner is configured.  Normal
    equations: every step is one plain product and one combined one, so half of the products are fused steps."""
    a, b = _child({"PRIMME_AMD_CHEB_FUSED": "1", "PRIMME_AMD_CHEB_UNFUSED": "0"}), _child({"PRIMME_AMD_CHEB_UNFUSED": "1"})
    for name in a:
        norm2 = GOLD[name]["norm2"]
        assert a[name]["ret"] == 0 and b[name]["ret"] == 0
        assert np.max(np.abs(np.array(a[name]["svals"]) - np.array(b[name]["svals"]))) <= 1e-10 * norm2
        assert abs(a[name]["its"] - b[name]["its"]) <= 1, (a[name], b[name])
        assert a[name]["stats"]["fused_steps"] > 0 and 2 * a[name]["stats"]["fused_steps"] == a[name]["stats"]["operator_products"]
        assert b[name]["stats"]["fused_steps"] == 0 and b[name]["stats"]["operator_products"] > 0


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_hip_against_the_checker(built, name):
    """backend="hip" with precond=("chebyshev", ...) against backend="hostcheck" with the numpy callback.  Without the feature the
    tuple selected Jacobi, there was no precond_stats and the counts were those of another preconditioner."""
    m, n, csr, kw, spec, dtype, norm2, tup = SC.case_setup(name)
    eps, d = kw["eps"], spec["steps"]
    r = SC.run_case(name, "hip")
    h = SC.run_case(name, "hostcheck")
    print(name, "outer", r.stats["numOuterIterations"], h.stats["numOuterIterations"], "preconds", r.stats["numPreconds"], r.precond_stats,
          "stage 1 preconds", r.eig_stats["numPreconds"])
    assert r.ret == 0 and h.ret == 0 and r.initSize == h.initSize == kw["numSvals"]
    assert np.max(np.abs(np.sort(np.asarray(r.svals, dtype=np.float64)) - np.sort(np.asarray(h.svals, dtype=np.float64)))) <= eps * norm2
    assert np.all(np.asarray(r.resNorms) <= eps * r.params["aNorm"] * (1 + 1e-6))
    its, itsh = r.stats["numOuterIterations"], h.stats["numOuterIterations"]
    assert abs(its - itsh) <= max(2, 0.02 * itsh), (its, itsh)
    assert r.precond_stats is not None and r.precond_stats["applies"] == r.stats["numPreconds"] > 0
    method = kw.get("method", "normalequations")
    if method == "normalequations":
        assert r.precond_stats["operator_products"] == 2 * (d - 1) * r.precond_stats["applies"]
    elif method == "augmented":
        assert r.precond_stats["operator_products"] == (4 * (d - 1) + 2) * r.precond_stats["applies"]
    else:
        # hybrid: the first stage runs the normal equations, the second the augmented operator; whatever the split, the count lies
        # between the two formulas and is one of the values a split of `applies` gives
        lo, hi = 2 * (d - 1) * r.precond_stats["applies"], (4 * (d - 1) + 2) * r.precond_stats["applies"]
        assert lo <= r.precond_stats["operator_products"] <= hi
        assert (r.precond_stats["operator_products"] - lo) % (2 * (d - 1) + 2) == 0


def test_capability_halves_the_outer_iterations(built):
    """D (200 columns), 3 smallest, normal equations, GD+k: 8 steps need at most half the outer iterations of the plain solve."""
    plain = SC.run_case("D200_s8", "hip", plain=True)
    pre = SC.run_case("D200_s8", "hip")
    print("outer iterations: plain", plain.stats["numOuterIterations"], "chebyshev", pre.stats["numOuterIterations"], pre.precond_stats)
    assert plain.ret == 0 and pre.ret == 0
    assert np.max(np.abs(plain.svals - pre.svals)) <= 1e-8 * 2.0
    assert 2 * pre.stats["numOuterIterations"] <= plain.stats["numOuterIterations"]
    assert plain.precond_stats is None


def test_set_chebyshev_argument_checks(built):
    m, n, csr = SC.difference_matrix(200)
    op = _Operator(m, n, csr, np.float64)
    lib = op.lib
    try:
        f = lib.primme_amd_svds_operator_set_chebyshev
        assert f(op.op, 0, 0.0, 2.0, 0.0) == -1
        assert f(op.op, 4, -0.1, 2.0, 0.0) == -1
        assert f(op.op, 4, math.nan, 2.0, 0.0) == -1
        assert f(op.op, 4, 2.0, 2.0, 0.0) == -1
        assert f(op.op, 4, 3.0, 2.0, 0.0) == -1
        assert f(op.op, 4, 0.1, 2.0, 1.0) == -1           # strictly inside
        assert f(op.op, 4, 0.1, 2.0, -0.05) == -1 and f(op.op, 4, 0.1, 2.0, -3.0) == -1     # singular value units: no negative shift
        assert f(op.op, 4, 0.1, 2.0, math.nan) == -1
        assert f(op.op, 4, 0.1, 2.0, 0.1) == 0            # at either end: allowed
        assert f(op.op, 4, 0.1, 2.0, 2.0) == 0
        assert f(op.op, 4, 0.1, 2.0, 0.0) == 0 and f(op.op, 4, 0.1, 2.0, 2.5) == 0
        b = C.c_double()
        assert lib.primme_amd_svds_operator_norm_bound(op.op, C.byref(b)) == 0 and b.value == 2.0
        # shi = NaN is that bound, 2.0 exactly: a shift just below it lies inside, the bound itself is an end; slo = 2 is no interval
        assert f(op.op, 4, 0.1, math.nan, 0.0) == 0
        assert f(op.op, 4, 0.1, math.nan, math.nextafter(2.0, 0.0)) == -1
        assert f(op.op, 4, 0.1, math.nan, 2.0) == 0
        assert f(op.op, 4, 2.0, math.nan, 0.0) == -1 and f(op.op, 4, math.nextafter(2.0, 0.0), math.nan, 0.0) == 0
    finally:
        op.close()


def test_row_partitioned_operator_is_refused(built):
    """-44, as primme_amd_svds_operator_set_jacobi answers: on the one-rank communicator tests/test_comm_gpu.py uses"""
    from test_comm_gpu import _comm
    lib = F.load_product()
    m, n, (rp, ci, va) = SC.difference_matrix(200)
    comm = _comm(lib)
    ctx, op = C.c_void_p(), C.c_void_p()
    assert lib.hipk_ctx_create(C.byref(ctx), None) == 0
    lib.primme_amd_svds_operator_create_dist.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_int64,
                                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    try:
        assert lib.primme_amd_svds_operator_create_dist(C.byref(op), ctx, F.HIPK_F64, m, n, n, rp.ctypes.data_as(C.c_void_p),
                                                        ci.ctypes.data_as(C.c_void_p), va.ctypes.data_as(C.c_void_p), comm) == 0
        assert lib.primme_amd_svds_operator_set_chebyshev(op, 4, 0.0, 2.0, 2.0) == -44
        b = C.c_double()
        assert lib.primme_amd_svds_operator_norm_bound(op, C.byref(b)) == -44
        lib.primme_amd_svds_operator_destroy(op)
    finally:
        lib.hipk_ctx_destroy(ctx)
        lib.primme_amd_comm_destroy(comm)
