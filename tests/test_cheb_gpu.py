"""The Chebyshev polynomial preconditioner on the MI355X: the kernels of csrc/hipk_cheb.hip and the fused steps against the
numpy recurrence (tests/cheb_cases.py), the fused path against the generic one, parity with the reference fixture
(tests/golden/reference_cheb.json), what the preconditioner buys, and the Gershgorin bounds."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cheb_cases as CC
import reference_driver_cases as RD
from checkers import Operator, eigsh
from primme_amd import _ffi as F
from primme_amd import problems

pytestmark = pytest.mark.gpu
GOLD = json.load(open(CC.GOLDEN))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACCURACY_LOG = os.path.join(ROOT, "profiles", "cheb_kernel_accuracy.txt")


@pytest.fixture(scope="module")
def accuracy_log():
    """The kernel cases add their figures; what the run observed goes to profiles/cheb_kernel_accuracy.txt when the module is
    done (only a run of the whole kernel sweep rewrites the record)."""
    lines = []
    yield lines
    if len(lines) >= 18:
        with open(ACCURACY_LOG, "w") as f:
            f.write("Chebyshev kernels against the spectral value U p(Lambda) U' x, 23 x 29 Laplacian, relative infinity norm\n")
            f.write("\n".join(lines) + "\n")


def _u(dtype):
    return 2.0 ** -53 if np.dtype(dtype) == np.float64 else 2.0 ** -24


class _Dev:
    """Panels in HBM through torch; leading dimensions differ from the row count and from each other."""

    def __init__(self):
        import torch
        self.torch = torch

    def panel(self, a, ld):
        t = self.torch.zeros((a.shape[1], ld), dtype=getattr(self.torch, str(a.dtype)), device="cuda")
        t[:, :a.shape[0]] = self.torch.from_numpy(np.ascontiguousarray(a.T)).to("cuda")
        return t

    def back(self, t, n):
        self.torch.cuda.synchronize()
        return t[:, :n].cpu().numpy().T.astype(np.float64)


def _coef(cy, cp, cx, cw):
    cf = F.HipkChebCoef()
    for c in range(len(cy)):
        cf.cy[c], cf.cp[c], cf.cx[c], cf.cw[c] = cy[c], cp[c], cx[c], cw[c]
    return cf


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _kernel_case(n_dims, nb, steps):
    """A, its spectrum, a block X and per-column shifts at or below lo."""
    rp, ci, va, n = problems.laplacian_csr(n_dims)
    A = CC.dense_of(rp, ci, va, n)
    lam, U = np.linalg.eigh(A)
    X = np.random.default_rng(11 + nb).standard_normal((n, nb))
    sig = np.linspace(-0.5, 0.2, nb) if nb > 1 else np.array([0.03])
    return (rp, ci, va, n), A, lam, U, X, sig


def _run_steps(lib, dev, form, csr, dtype, X, sig, steps, lo, hi, lds4=None):
    """y_steps through the device: form "update" = numpy-independent operator product by hipk_csr_matvec + hipk_cheb_update,
    "pat" / "csr" = hipk_csr_cheb_step on the row-pattern / row-tile form.  y_1 = x/tb is formed by hipk_cheb_update."""
    rp, ci, va, n = csr
    nb = X.shape[1]
    dt = F.HIPK_F64 if np.dtype(dtype) == np.float64 else F.HIPK_F32
    ctx, Ah = C.c_void_p(), C.c_void_p()
    assert lib.hipk_ctx_create(C.byref(ctx), None) == 0
    vat = np.ascontiguousarray(va, dtype=dtype)
    assert lib.hipk_csr_create(ctx, dt, n, n, 0, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p), vat.ctypes.data_as(C.c_void_p), C.byref(Ah)) == 0
    old = lib.hipk_set_spmv_format(1 if form == "pat" else 0)
    lx, l0, l1, lw = lds4 or (n + 3, n + 5, n + 8, n + 13)
    try:
        # the form under test is the one that runs: 2 = row patterns, 0 = CSR row tiles
        if form != "update":
            assert lib.hipk_csr_format(Ah) == (2 if form == "pat" else 0)
        st = lib.hipk_ctx_stream(ctx)
        Xd = dev.panel(X.astype(dtype), lx)
        Y = [dev.panel(np.zeros((n, nb), dtype=dtype), l0), dev.panel(np.zeros((n, nb), dtype=dtype), l1)]
        W = dev.panel(np.zeros((n, nb), dtype=dtype), lw)
        tb, coef = CC.cheb_step_coefficients(steps, lo, hi, sig)
        z = np.zeros(nb)
        assert lib.hipk_cheb_update(st, dt, n, nb, C.byref(_coef(z, z, 1.0 / tb, z)), _ptr(Xd), lx, None, 0, None, 0, None, 0, _ptr(Y[0]), l0) == 0
        lds = [l0, l1]
        k, p = 0, 1          # y_k in Y[k], y_{k-1} in Y[p] (zero at the first step)
        for cy, cp, cx, cw in coef:
            cf = _coef(cy, cp + z, cx, cw)
            if form == "update":
                assert lib.hipk_csr_matvec(Ah, st, _ptr(Y[k]), lds[k], _ptr(W), lw, nb) == 0
                assert lib.hipk_cheb_update(st, dt, n, nb, C.byref(cf), _ptr(Xd), lx, _ptr(W), lw, _ptr(Y[k]), lds[k], _ptr(Y[p]), lds[p],
                                            _ptr(Y[p]), lds[p]) == 0
            else:
                assert lib.hipk_csr_cheb_step(Ah, st, nb, C.byref(cf), _ptr(Xd), lx, _ptr(Y[k]), lds[k], _ptr(Y[p]), lds[p], _ptr(Y[p]), lds[p]) == 0
            k, p = p, k
        assert lib.hipk_sync(ctx) == 0
        return dev.back(Y[k], n)
    finally:
        lib.hipk_set_spmv_format(old)
        lib.hipk_csr_destroy(Ah)
        lib.hipk_ctx_destroy(ctx)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("nb", [1, 3, 8])
@pytest.mark.parametrize("form", ["update", "pat", "csr"])
def test_kernels_against_the_recurrence(built, accuracy_log, form, nb, dtype):
    """E = distance of the float64 numpy recurrence from the spectral value on the same input; the device result must lie
    within max(8 E, 64 d u_T) of the spectral value (8: another summation order in the row sums; 64 d u: the floor when E is
    at roundoff).  23 x 29 rows: not a multiple of the workgroup's rows; ldx != ldy != m; distinct shifts per column."""
    lib = F.load_product()
    dev = _Dev()
    steps, lo, hi = 8, 0.25, 8.0
    csr, A, lam, U, X, sig = _kernel_case((23, 29), nb, steps)
    Xt = X.astype(dtype).astype(np.float64)             # the input the device sees
    spectral = np.stack([CC.cheb_spectral(lam, U, Xt[:, c], steps, lo, hi, sig[c]) for c in range(nb)], axis=1)
    E = CC.rel_inf(CC.cheb_recurrence(lambda v: A @ v, Xt, steps, lo, hi, sig), spectral)
    got = _run_steps(lib, dev, form, csr, dtype, X, sig, steps, lo, hi)
    D = CC.rel_inf(got, spectral)
    bound = max(8 * E, 64 * steps * _u(dtype))
    line = f"{form:6s} {np.dtype(dtype).name:8s} nb={nb} steps={steps}  E(numpy recurrence)={E:.3e}  device distance={D:.3e}  bound={bound:.3e}"
    print(line)
    accuracy_log.append(line)
    assert D <= bound, line


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_update_kernel_wide_accesses_with_a_tail(built, dtype):
    """The same check on panels whose columns all start on 16-byte boundaries (torch allocations are 256-byte aligned, the
    leading dimensions are multiples of 4 elements), so hipk_cheb_update takes its 16-byte path with all four inputs, and
    667 rows = 23 x 29 are no multiple of the elements per access (2 for double, 4 for float): the scalar tail runs too."""
    lib = F.load_product()
    dev = _Dev()
    steps, lo, hi, nb = 8, 0.25, 8.0, 3
    csr, A, lam, U, X, sig = _kernel_case((23, 29), nb, steps)
    n = csr[3]
    assert n % 2 == 1
    Xt = X.astype(dtype).astype(np.float64)
    spectral = np.stack([CC.cheb_spectral(lam, U, Xt[:, c], steps, lo, hi, sig[c]) for c in range(nb)], axis=1)
    E = CC.rel_inf(CC.cheb_recurrence(lambda v: A @ v, Xt, steps, lo, hi, sig), spectral)
    got = _run_steps(lib, dev, "update", csr, dtype, X, sig, steps, lo, hi, lds4=(n + 1, n + 5, n + 9, n + 13))
    D = CC.rel_inf(got, spectral)
    bound = max(8 * E, 64 * steps * _u(dtype))
    print(f"aligned {np.dtype(dtype).name} E={E:.3e} device distance={D:.3e} bound={bound:.3e}")
    assert D <= bound


def test_complex_update_kernel(built):
    """hipk_cheb_update on complex panels (real coefficients) against numpy."""
    lib = F.load_product()
    dev = _Dev()
    n, nb = 1001, 3
    rng = np.random.default_rng(2)
    arrs = [(rng.standard_normal((n, nb)) + 1j * rng.standard_normal((n, nb))) for _ in range(4)]
    cy, cp, cx, cw = (rng.standard_normal(nb) for _ in range(4))
    for dtype, dt in ((np.complex128, F.HIPK_C64), (np.complex64, F.HIPK_C32)):
        X, W, Yk, Yp = (a.astype(dtype) for a in arrs)
        want = cy * Yk.astype(np.complex128) + cp * Yp.astype(np.complex128) + cx * X.astype(np.complex128) + cw * W.astype(np.complex128)
        ts = [dev.panel(a, n + 1 + i) for i, a in enumerate((X, W, Yk, Yp))]
        assert lib.hipk_cheb_update(None, dt, n, nb, C.byref(_coef(cy, cp, cx, cw)), _ptr(ts[0]), n + 1, _ptr(ts[1]), n + 2, _ptr(ts[2]), n + 3,
                                    _ptr(ts[3]), n + 4, _ptr(ts[3]), n + 4) == 0
        dev.torch.cuda.synchronize()
        got = ts[3][:, :n].cpu().numpy().T
        u = 2.0 ** -53 if dtype == np.complex128 else 2.0 ** -24
        assert np.max(np.abs(got - want)) <= 16 * u * np.max(np.abs(want))


def test_set_chebyshev_argument_checks(built):
    import math
    from checkers import Session
    rp, ci, va, n = problems.laplacian_csr((8, 9))
    s = Session(Operator(n, csr=(rp, ci, va)), backend="hip")
    try:
        f = s.lib.primme_amd_operator_set_chebyshev
        assert f(s.oph, 0, 0.1, 8.0, 0, 0.0) == -1
        assert f(s.oph, 4, 8.0, 8.0, 0, 0.0) == -1
        assert f(s.oph, 4, 9.0, 8.0, 0, 0.0) == -1
        assert f(s.oph, 4, math.nan, 8.0, 0, 0.0) == -1
        assert f(s.oph, 4, 0.1, 8.0, 1, 3.0) == -1          # fixed shift strictly inside
        assert f(s.oph, 4, 0.1, 8.0, 1, 0.1) == 0           # at the end: allowed
        assert f(s.oph, 4, 0.1, 8.0, 1, -1.0) == 0
        assert f(s.oph, 4, 0.1, math.nan, 0, 0.0) == 0      # hi from Gershgorin
        with pytest.raises(ValueError):
            s.solve(numEvals=1, precond=("chebyshev", 4, 9.0, 8.0))
        for bad in (("chebyshev",), ("chebyshev", 4), ("chebyshev", 4, 0.1, 8.0, -1.0, 0.0)):      # malformed tuples
            with pytest.raises(ValueError, match="steps, lo"):
                s.solve(numEvals=1, precond=bad)
        # solver shifts serve the extremal targets only: the callback refuses, the solve ends with the user-failure code
        r = s.solve(numEvals=1, target="closest_abs", targetShifts=[1.0], precond=("chebyshev", 4, 0.1, 8.0), aNorm=8.0)
        assert r.ret == -41
    finally:
        s.close()


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_hip_against_reference_fixture(built, name):
    g = GOLD[name]
    r = CC.run_case(name, "hip")
    aN = g["aNorm"]
    rel = 1e-4 if CC.CASES[name].get("dtype") == "float32" else 1e-10
    assert r.ret == 0 and r.initSize == g["initSize"]
    assert np.max(np.abs(np.sort(np.asarray(r.evals, dtype=np.float64)) - np.sort(np.array(g["evals"])))) <= rel * aN
    assert np.all(np.asarray(r.resNorms) <= CC.CASES[name]["kw"]["eps"] * aN * (1 + 1e-6))
    its, itsg = r.stats["numOuterIterations"], g["stats"]["numOuterIterations"]
    print(name, "outer", its, itsg, "preconds", r.stats["numPreconds"], g["stats"]["numPreconds"], r.precond_stats)
    # the band tests/test_solver_gpu.py gives preconditioned fixtures at block size 1 and in the Davidson family
    assert abs(its - itsg) <= max(2, 0.02 * itsg), (its, itsg)
    assert abs(r.precond_stats["applies"] - g["precond_applies"]) <= max(2, 0.02 * g["precond_applies"])
    assert r.precond_stats["applies"] == r.stats["numPreconds"]
    assert r.precond_stats["operator_products"] == (g["cheb"]["steps"] - 1) * r.precond_stats["applies"]


_CHILD = r"""
import json, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + "/oracle"); sys.path.insert(0, {root!r} + "/tests")
import numpy as np
import cheb_cases as CC
out = {{}}
for name in ("gdk_60x61_s8", "olsen_b4"):
    r = CC.run_case(name, "hip")
    out[name] = dict(ret=r.ret, evals=np.asarray(r.evals).tolist(), its=r.stats["numOuterIterations"], stats=r.precond_stats)
print("RESULT " + json.dumps(out))
"""


def _child(env_extra):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def test_fused_against_generic(built):
    """The same solves with the fused steps and with PRIMME_AMD_CHEB_UNFUSED=1 (each in a fresh process: the knob is read when
    the preconditioner is configured): same eigenvalues to 1e-10 |A|, outer iterations within 1."""
    a, b = _child({"PRIMME_AMD_CHEB_UNFUSED": "0"}), _child({"PRIMME_AMD_CHEB_UNFUSED": "1"})
    for name in a:
        assert a[name]["ret"] == 0 and b[name]["ret"] == 0
        assert np.max(np.abs(np.array(a[name]["evals"]) - np.array(b[name]["evals"]))) <= 1e-10 * 8.0
        assert abs(a[name]["its"] - b[name]["its"]) <= 1, (a[name], b[name])
        assert a[name]["stats"]["fused_steps"] > 0 and a[name]["stats"]["fused_steps"] == a[name]["stats"]["operator_products"]
        assert b[name]["stats"]["fused_steps"] == 0 and b[name]["stats"]["operator_products"] > 0


def test_capability_halves_the_outer_iterations(built):
    """60 x 61 Laplacian, 3 smallest, GD+k, eps 1e-8: ("chebyshev", 8, 0.1) — hi from Gershgorin — needs at most half the outer
    iterations of the unpreconditioned solve (a dense numpy Davidson sketch gives 48 against 330)."""
    rp, ci, va, n = problems.laplacian_csr((60, 61))
    op = Operator(n, csr=(rp, ci, va))
    kw = dict(numEvals=3, method="GD_plusK", eps=1e-8, aNorm=8.0, v0=problems.start_vector(n))
    plain = eigsh(op, backend="hip", **kw)
    pre = eigsh(op, backend="hip", precond=("chebyshev", 8, 0.1), **kw)
    print("outer iterations: plain", plain.stats["numOuterIterations"], "chebyshev", pre.stats["numOuterIterations"], pre.precond_stats)
    assert plain.ret == 0 and pre.ret == 0
    assert np.max(np.abs(plain.evals - pre.evals)) <= 1e-10 * 8.0
    assert 2 * pre.stats["numOuterIterations"] <= plain.stats["numOuterIterations"]
    assert pre.precond_stats["operator_products"] == 7 * pre.precond_stats["applies"]
    assert plain.precond_stats is None


def _gershgorin(op, dtype=np.float64):
    from checkers import Session
    s = Session(op, backend="hip", dtype=dtype)
    try:
        lo, hi = C.c_double(), C.c_double()
        assert s.lib.primme_amd_operator_gershgorin(s.oph, C.byref(lo), C.byref(hi)) == 0
        return lo.value, hi.value
    finally:
        s.close()


def test_gershgorin(built):
    rp, ci, va, n = RD.lunda()
    lo, hi = _gershgorin(Operator(n, csr=(rp, ci, va)))
    lam = np.linalg.eigvalsh(CC.dense_of(rp, ci, va, n))
    glo, ghi = CC.gershgorin_numpy(rp, ci, va, n)
    assert lo <= lam[0] and lam[-1] <= hi
    nnz_row = int(np.max(np.diff(rp)))
    scale = max(abs(glo), abs(ghi))
    assert abs(lo - glo) <= 8 * nnz_row * 2.0 ** -53 * scale and abs(hi - ghi) <= 8 * nnz_row * 2.0 ** -53 * scale
    assert _gershgorin(Operator(40 * 41, stencil=(40, 41, 1))) == (0.0, 8.0)
    rp, ci, va, n = problems.laplacian_csr((40, 41))
    assert _gershgorin(Operator(n, csr=(rp, ci, va))) == (0.0, 8.0)
    rp, ci, va = problems.hermitian_banded_csr(300)[:3]
    lo, hi = _gershgorin(Operator(300, csr=(rp, ci, va)), dtype=np.complex128)
    lam = np.linalg.eigvalsh(CC.dense_of(rp, ci, va, 300))
    assert lo <= lam[0] and lam[-1] <= hi
