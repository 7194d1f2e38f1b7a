"""Thin Python driver over the C ABI (plumbing only: memory, handles, parameter block).

`Session` keeps a sparse operator resident in HBM and runs hip_dprimme / hip_sprimme /
hip_zprimme / hip_cprimme solves on it; `eigsh(...)` is the one-shot form.  This package loads the
product library only (primme_amd/libprimme_amd.so).  Test code can drive the very same parameter
plumbing over another library by passing a *backend object* (see `HipBackend` for the interface);
the checker back ends live under oracle/ (oracle/checkers.py) and are never imported from here.
"""
import ctypes as C
import hashlib

import numpy as np

from . import _ffi as F
from .members import apply_members


class Operator:
    """A sparse operator: CSR arrays (global column indices) or a Laplacian stencil,
    rows [row0, row0+nrows) of an n x n matrix.

    diag_patterns=True (real CSR matrices): when the rows repeat but for their diagonal entry (stencil or lattice operator +
    potential / on-site term), the device keeps one byte per row and streams the diagonal (HIPK_CSR_DIAG_PATTERNS of
    hipk_csr_create_opts) instead of the CSR arrays for the one-column products; same results, fewer bytes.

    sliced=True (real CSR matrices without halo): a general matrix also gets the sliced-ELL form (HIPK_CSR_SLICED) that serves
    the plain and the shifted products of any width, when its padding stays within 1.25 nnz; the CSR arrays stay on the device
    beside it.  Results agree with the row tiles' to rounding.  Both keywords may be set."""

    def __init__(self, n, csr=None, stencil=None, row0=0, nrows=None, diag_patterns=False, sliced=False):
        self.n = int(n)
        self.diag_patterns = bool(diag_patterns)
        self.sliced = bool(sliced)
        self.csr = csr            # (rowptr int32, colind int32, values)
        self.stencil = stencil    # (nx, ny, nz)
        self.row0 = int(row0)
        self.nrows = int(nrows if nrows is not None else (len(csr[0]) - 1 if csr is not None else n))

    def apply_numpy(self, x):
        from .problems import csr_matvec_numpy, laplacian_csr
        if self.csr is None:
            dims = tuple(d for d in self.stencil if d and d > 0)
            self.csr = laplacian_csr(dims, self.row0, self.nrows)[:3]
        assert self.nrows == self.n, "numpy apply is single-rank only"
        return csr_matvec_numpy(self.csr[0], self.csr[1], self.csr[2], x)

    def diagonal(self):
        if self.csr is None:
            d = len([x for x in self.stencil if x and x > 1])
            return np.full(self.nrows, 2.0 * max(d, 1))
        rp, ci, va = self.csr
        va = np.real(va)
        rows = np.repeat(np.arange(self.nrows), np.diff(rp))
        dg = np.zeros(self.nrows)
        m = ci == rows + self.row0
        dg[rows[m]] = va[m]
        return dg


class Result:
    def __init__(self, ret, evals, evecs, resNorms, params):
        self.ret, self.evals, self.evecs, self.resNorms = ret, evals, evecs, resNorms
        self.initSize = params.initSize
        s = params.stats
        self.stats = {k: getattr(s, k) for k, _ in F.PrimmeStats._fields_}
        self.params = {k: getattr(params, k) for k in ("maxBasisSize", "minRestartSize", "maxBlockSize",
                                                       "locking", "orth", "aNorm", "eps", "initSize", "dynamicMethodSwitch")}
        self.params["maxPrevRetain"] = params.restartingParams.maxPrevRetain
        # Chebyshev preconditioner: {"applies", "operator_products", "fused_steps"} of this solve (counted in vectors);
        # multigrid preconditioner: {"applies", "launches"} (vectors, kernel launches); algebraic multigrid: {"applies",
        # "launches", "levels"}
        self.precond_stats = None


class HipBackend:
    """The product: libprimme_amd.so, vectors in HBM (torch tensors hold the device memory)."""
    name = "hip"
    device = True            # evecs live in HBM
    native_operator = True   # the library's own operator handle / ready-made callbacks are used

    def __init__(self):
        self.lib = F.load_product()

    def solver(self, dtype_name):
        return getattr(self.lib, {"float64": "hip_dprimme", "float32": "hip_sprimme", "complex128": "hip_zprimme",
                                  "complex64": "hip_cprimme"}[dtype_name])

    def svds_solver(self, dtype_name):
        return getattr(self.lib, {"float64": "hip_dprimme_svds", "float32": "hip_sprimme_svds", "complex128": "hip_zprimme_svds",
                                  "complex64": "hip_cprimme_svds"}[dtype_name])


def _resolve_backend(backend):
    if backend == "hip":
        return HipBackend()
    if isinstance(backend, str):
        raise ValueError(f"backend {backend!r}: primme_amd has one back end, the MI355X library; the CPU checkers "
                         "used by the tests are constructed by oracle/checkers.py")
    return backend


class Session:
    def __init__(self, op, comm=None, dtype=np.float64, backend="hip", complex_form="native", mass=None):
        self.op, self.comm = op, comm
        self.mass = mass         # Operator of the mass matrix B of a generalised problem A x = lambda B x (real, CSR), or None
        self.mass_oph = None
        self.be = _resolve_backend(backend)
        self.backend = self.be.name
        self.dtype = np.dtype(dtype)
        # Hermitian problems: complex vectors (csrc/eigs_complex.c)
        self.cplx = self.dtype.kind == "c"
        self.rdtype = np.dtype(np.float64 if self.dtype in (np.float64, np.complex128) else np.float32)
        self.dt = F.HIPK_F64 if self.rdtype == np.float64 else F.HIPK_F32
        self.handles = []
        self.keep = []
        self._v0_cache = None
        self.lib = self.be.lib
        if not self.be.native_operator:
            return
        lib = self.lib
        ctx = C.c_void_p()
        if lib.hipk_ctx_create(C.byref(ctx), None):
            raise RuntimeError("hipk_ctx_create failed: no HIP device (primme_amd has no CPU path)")
        self.handles.append(("ctx", ctx))
        A = C.c_void_p()
        if op.csr is not None:
            rp, ci, va = op.csr
            rp = np.ascontiguousarray(rp, dtype=np.int32)
            ci = np.ascontiguousarray(ci, dtype=np.int32)
            self.real_form = self.cplx and complex_form != "native"
            if self.cplx and not self.real_form:
                # a complex CSR matrix on the device: hip_zprimme / hip_cprimme run natively on complex panels
                vz = np.ascontiguousarray(va, dtype=self.dtype)
                cdt = F.HIPK_C64 if self.dtype == np.complex128 else F.HIPK_C32
                rc = lib.hipk_csr_create(ctx, cdt, op.nrows, op.n, op.row0, rp.ctypes.data_as(C.c_void_p),
                                         ci.ctypes.data_as(C.c_void_p), vz.ctypes.data_as(C.c_void_p), C.byref(A))
            elif self.cplx:
                # the real-equivalent 2n x 2n expansion (csrc/eigs_complex.c): what extractions / methods without
                # complex objects fall back to
                vz = np.ascontiguousarray(va, dtype=np.complex128)
                rp2, ci2, va2 = C.c_void_p(), C.c_void_p(), C.c_void_p()
                rc = lib.primme_amd_csr_complex_to_real(op.nrows, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                                        vz.ctypes.data_as(C.c_void_p), C.byref(rp2), C.byref(ci2), C.byref(va2))
                if rc:
                    raise RuntimeError(f"real-equivalent expansion failed: {rc}")
                nnz2 = 4 * int(rp[-1])
                v2 = np.ctypeslib.as_array(C.cast(va2, C.POINTER(C.c_double)), shape=(max(nnz2, 1),)).astype(self.rdtype)
                rc = lib.hipk_csr_create(ctx, self.dt, 2 * op.nrows, 2 * op.n, 2 * op.row0, rp2, ci2, v2.ctypes.data_as(C.c_void_p), C.byref(A))
                for h in (rp2, ci2, va2): lib.primme_amd_host_free(h)
            else:
                va = np.ascontiguousarray(va, dtype=self.dtype)
                flags = ((F.HIPK_CSR_DIAG_PATTERNS if getattr(op, "diag_patterns", False) else 0) |
                         (F.HIPK_CSR_SLICED if getattr(op, "sliced", False) else 0))
                if flags and self.be.device:
                    # the form of the device operator only: a checker that runs the host solver over host vectors has one form
                    rc = lib.hipk_csr_create_opts(ctx, self.dt, op.nrows, op.n, op.row0, rp.ctypes.data_as(C.c_void_p),
                                                  ci.ctypes.data_as(C.c_void_p), va.ctypes.data_as(C.c_void_p),
                                                  flags, C.byref(A))
                else:
                    rc = lib.hipk_csr_create(ctx, self.dt, op.nrows, op.n, op.row0, rp.ctypes.data_as(C.c_void_p),
                                             ci.ctypes.data_as(C.c_void_p), va.ctypes.data_as(C.c_void_p), C.byref(A))
        else:
            nx, ny, nz = (list(op.stencil) + [1, 1])[:3]
            rc = lib.hipk_stencil_create(ctx, self.dt, nx, ny or 1, nz or 1, op.row0, op.nrows, C.byref(A))
        if rc:
            raise RuntimeError(f"operator creation failed: {rc}")
        self.handles.append(("csr", A))
        oph = C.c_void_p()
        if lib.primme_amd_operator_create(C.byref(oph), A, comm):
            raise RuntimeError("operator handle creation failed")
        self.handles.append(("op", oph))
        if self.cplx and self.real_form: lib.primme_amd_operator_set_complex(oph, 1)
        self.oph = oph
        if mass is not None:
            if (self.cplx and self.real_form) or mass.csr is None:
                raise ValueError("mass matrix: CSR operators, complex ones on the native complex panels")
            rpb, cib, vab = mass.csr
            rpb = np.ascontiguousarray(rpb, dtype=np.int32); cib = np.ascontiguousarray(cib, dtype=np.int32)
            vab = np.ascontiguousarray(vab, dtype=self.dtype)
            Bh = C.c_void_p()
            bdt = self.dt if not self.cplx else (F.HIPK_C64 if self.dtype == np.complex128 else F.HIPK_C32)
            if lib.hipk_csr_create(ctx, bdt, mass.nrows, mass.n, mass.row0, rpb.ctypes.data_as(C.c_void_p),
                                   cib.ctypes.data_as(C.c_void_p), vab.ctypes.data_as(C.c_void_p), C.byref(Bh)):
                raise RuntimeError("mass matrix creation failed")
            self.handles.append(("csr", Bh))
            ophB = C.c_void_p()
            if lib.primme_amd_operator_create(C.byref(ophB), Bh, comm):
                raise RuntimeError("mass operator handle creation failed")
            self.handles.append(("op", ophB))
            self.mass_oph = ophB

    def close(self):
        for kind, h in reversed(self.handles):
            if kind == "op": self.lib.primme_amd_operator_destroy(h)
            elif kind == "csr": self.lib.hipk_csr_destroy(h)
            elif kind == "ctx": self.lib.hipk_ctx_destroy(h)
        self.handles = []

    def solve(self, numEvals=1, target="smallest", method="GD_plusK", eps=1e-8, aNorm=0.0, v0=None,
              maxBlockSize=0, maxBasisSize=0, minRestartSize=0, maxPrevRetain=None, locking=None,
              maxMatvecs=0, maxOuterIterations=0, targetShifts=None, precond=None, printLevel=0,
              initBasisMode=None, global_sum=None, numProcs=1, procID=0, orth=None, iseed=None,
              profile=False, return_evecs=True, monitor=None, user_matvec=None, projection=None,
              constraints=None, user_precond=None, tweak=None, members=None):
        lib, op, dtype = self.lib, self.op, self.dtype
        keep = []
        cheb = isinstance(precond, (tuple, list)) and len(precond) > 0 and precond[0] == "chebyshev"
        if cheb:
            if not 3 <= len(precond) <= 5:
                raise ValueError("precond: ('chebyshev', steps, lo[, hi[, shift]])")
            if not (self.be.native_operator and hasattr(lib, "primme_amd_chebyshev_precond")):
                raise ValueError(f"precond={precond!r}: the Chebyshev preconditioner applies the device operator of the product "
                                 f"library; back end {self.backend!r} has no such operator")
            if user_precond is not None:
                raise ValueError("precond=('chebyshev', ...) and user_precond exclude each other")
        mg = isinstance(precond, (tuple, list)) and len(precond) > 0 and precond[0] == "multigrid"
        if mg:
            if not 2 <= len(precond) <= 6:
                raise ValueError("precond: ('multigrid', dims[, smooth_steps[, coarse_steps[, scale[, shift]]]])")
            if not (self.be.native_operator and hasattr(lib, "primme_amd_multigrid_precond")):
                raise ValueError(f"precond={precond!r}: the multigrid preconditioner runs on the device operator of the product "
                                 f"library; back end {self.backend!r} has no such operator")
            if user_precond is not None:
                raise ValueError("precond=('multigrid', ...) and user_precond exclude each other")
            if self.cplx:
                raise ValueError(f"precond={precond!r}: the multigrid preconditioner serves real operators")
            if self.comm is not None:
                raise ValueError(f"precond={precond!r}: the multigrid preconditioner serves single-rank operators")
        amg = isinstance(precond, (tuple, list)) and len(precond) > 0 and precond[0] in ("amg", "amg_smoothed")
        smoothed = amg and precond[0] == "amg_smoothed"
        if amg:
            if not 1 <= len(precond) <= 6:
                raise ValueError(f"precond: ('{precond[0]}'[, smooth_steps[, coarse_steps[, theta[, {'omega' if smoothed else 'over'}[, shift]]]]])")
            if not (self.be.native_operator and hasattr(lib, "primme_amd_amg_precond")):
                raise ValueError(f"precond={precond!r}: the algebraic multigrid preconditioner runs on the device operator of the "
                                 f"product library; back end {self.backend!r} has no such operator")
            if user_precond is not None:
                raise ValueError(f"precond=('{precond[0]}', ...) and user_precond exclude each other")
            if self.cplx:
                raise ValueError(f"precond={precond!r}: the algebraic multigrid preconditioner serves real operators")
            if self.comm is not None:
                raise ValueError(f"precond={precond!r}: the algebraic multigrid preconditioner serves single-rank operators")
            if op.csr is None:
                raise ValueError(f"precond={precond!r}: the algebraic multigrid preconditioner reads the CSR arrays of the operator; "
                                 "a stencil operator has precond=('multigrid', dims)")
        amgh = isinstance(precond, (tuple, list)) and len(precond) > 0 and precond[0] == "amg_hierarchy"
        if amgh:
            # every argument error before any library call
            if not 2 <= len(precond) <= 5:
                raise ValueError("precond: ('amg_hierarchy', H[, smooth_steps[, coarse_steps[, over]]])")
            H = precond[1]
            if not isinstance(H, AmgHierarchy):
                raise ValueError(f"precond={precond!r}: the second entry is an AmgHierarchy")
            if H.closed:
                raise ValueError("precond=('amg_hierarchy', H): H is closed")
            h_nu = int(precond[2]) if len(precond) > 2 else 2
            h_ncs = int(precond[3]) if len(precond) > 3 else 16
            h_over = float(precond[4]) if len(precond) > 4 else 1.0
            if h_nu < 1 or h_ncs < 1 or not 1.0 <= h_over < 2.0:
                raise ValueError("precond=('amg_hierarchy', ...): needs steps >= 1 and 1 <= over < 2")
            if H.smoothed and h_over != 1.0:
                raise ValueError("precond=('amg_hierarchy', ...): over must be 1 with a smoothed hierarchy")
            if user_precond is not None:
                raise ValueError("precond=('amg_hierarchy', ...) and user_precond exclude each other")
            if self.cplx or self.comm is not None or op.csr is None:
                raise ValueError("precond=('amg_hierarchy', ...): the algebraic multigrid preconditioner serves real single-rank CSR operators")
            if (op.nrows, int(op.csr[0][-1])) != (H.n, H.matrix_nnz):
                raise ValueError(f"precond=('amg_hierarchy', H): H was built from a matrix of {H.n} rows and {H.matrix_nnz} entries, "
                                 f"the operator has {op.nrows} and {int(op.csr[0][-1])}")
            if not (self.be.native_operator and hasattr(lib, "primme_amd_operator_set_amg_hierarchy")):
                raise ValueError(f"precond=('amg_hierarchy', ...): the algebraic multigrid preconditioner runs on the device operator of "
                                 f"the product library; back end {self.backend!r} has no such operator")
        p = F.PrimmeParams()
        nLocal = op.nrows
        v0 = None if v0 is None else np.asarray(v0, dtype=dtype).reshape(nLocal, -1)
        initSize = 0 if v0 is None else v0.shape[1]
        if initBasisMode is None and v0 is not None:
            initBasisMode = F.primme_init_user

        lib.primme_initialize(C.byref(p))
        p.n = op.n
        p.numEvals = numEvals
        p.target = F.TARGETS[target] if isinstance(target, str) else target
        p.eps, p.aNorm, p.printLevel, p.outputFile = eps, aNorm, printLevel, None
        if maxBlockSize: p.maxBlockSize = maxBlockSize
        if maxBasisSize: p.maxBasisSize = maxBasisSize
        if minRestartSize: p.minRestartSize = minRestartSize
        if maxPrevRetain is not None: p.restartingParams.maxPrevRetain = maxPrevRetain
        if locking is not None: p.locking = locking
        if maxMatvecs: p.maxMatvecs = maxMatvecs
        if maxOuterIterations: p.maxOuterIterations = maxOuterIterations
        if orth is not None: p.orth = orth
        if projection is not None:
            p.projectionParams.projection = {"RR": 1, "harmonic": 2, "refined": 3}[projection]
        if iseed is not None:
            for i in range(4): p.iseed[i] = iseed[i]
        if targetShifts is not None:
            ts = (C.c_double * len(targetShifts))(*targetShifts)
            keep.append(ts)
            p.targetShifts, p.numTargetShifts = ts, len(targetShifts)
        p.initSize = initSize
        # orthogonality constraints: the first numOrthoConst columns of evecs (primme_eigs.h:266-269)
        cons = None if constraints is None else np.asarray(constraints, dtype=dtype).reshape(nLocal, -1)
        nOC = 0 if cons is None else cons.shape[1]
        p.numOrthoConst = nOC
        if initBasisMode is not None: p.initBasisMode = initBasisMode
        p.numProcs, p.procID, p.nLocal = numProcs, procID, nLocal
        m = F.METHODS[method] if isinstance(method, str) else method
        ncols = nOC + max(numEvals, initSize)
        ctype = C.c_double if self.rdtype == np.float64 else C.c_float
        cplx = self.cplx
        evecs_t = None

        def view(ptr, nb, ld):
            a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(nb, ld * (2 if cplx else 1)))
            return a.view(dtype) if cplx else a

        if not self.be.native_operator:
            # a checker that brings its own operator callbacks (oracle/checkers.py)
            evecs, evecs_ptr = self.be.setup_operator(self, p, keep, precond, view, ncols, nLocal, cons, nOC, v0, initSize)
            solver = self.be.solver(dtype.name)
        else:
            p.matrix = self.oph
            p.matrixMatvec = C.cast(lib.primme_amd_matvec, C.c_void_p)
            if self.mass_oph is not None:    # generalised problem: B through the ready-made callback over a second operator handle
                p.massMatrix = self.mass_oph
                p.massMatrixMatvec = C.cast(lib.primme_amd_mass_matvec, C.c_void_p)
            if user_matvec is not None:      # an application callback instead of the ready-made one
                keep.append(user_matvec)
                p.matrixMatvec = C.cast(user_matvec, C.c_void_p)
            if user_precond is not None:     # an application preconditioner callback (same pointer conventions as the matvec)
                keep.append(user_precond)
                p.applyPreconditioner = C.cast(user_precond, C.c_void_p)
                p.correctionParams.precondition = 1
            elif cheb:
                # ("chebyshev", steps, lo[, hi]): the solver's shifts; ("chebyshev", steps, lo, hi, shift): fixed shift.
                # hi left out (or None): the Gershgorin upper bound of the operator
                steps, lo = int(precond[1]), float(precond[2])
                hi = float("nan") if len(precond) < 4 or precond[3] is None else float(precond[3])
                fixed = len(precond) == 5
                if lib.primme_amd_operator_set_chebyshev(self.oph, steps, lo, hi, int(fixed), float(precond[4]) if fixed else 0.0):
                    raise ValueError(f"precond={precond!r}: needs steps >= 1, lo < hi and a fixed shift outside (lo, hi)")
                lib.primme_amd_chebyshev_stats(None, None, None)      # the counters are per process: start this solve at zero
                p.preconditioner = self.oph
                p.applyPreconditioner = C.cast(lib.primme_amd_chebyshev_precond, C.c_void_p)
                p.correctionParams.precondition = 1
            elif mg:
                # ("multigrid", dims[, smooth_steps[, coarse_steps[, scale[, shift]]]]): one V-cycle for scale * Laplacian + shift
                dims = tuple(int(d) for d in precond[1])
                if not 1 <= len(dims) <= 3:
                    raise ValueError(f"precond={precond!r}: dims holds one to three grid lengths, x first")
                nx, ny, nz = (list(dims) + [1, 1])[:3]
                nu = int(precond[2]) if len(precond) > 2 else 2
                ncs = int(precond[3]) if len(precond) > 3 else 16
                scale = float(precond[4]) if len(precond) > 4 else 1.0
                shift = float(precond[5]) if len(precond) > 5 else 0.0
                rc = lib.primme_amd_operator_set_multigrid(self.oph, nx, ny, nz, nu, ncs, scale, shift)
                if rc:
                    raise ValueError(f"precond={precond!r}: needs a real single-rank operator ({rc}), prod(dims) = its rows, "
                                     "steps >= 1, scale > 0 and shift >= 0")
                lib.primme_amd_multigrid_stats(None, None)            # the counters are per process: start this solve at zero
                p.preconditioner = self.oph
                p.applyPreconditioner = C.cast(lib.primme_amd_multigrid_precond, C.c_void_p)
                p.correctionParams.precondition = 1
            elif amg:
                # ("amg"[, smooth_steps[, coarse_steps[, theta[, over[, shift]]]]]): one V-cycle for A + shift on the hierarchy
                # that the library aggregates from the operator's own CSR arrays; ("amg_smoothed", ..., omega, shift): the
                # same with smoothed prolongations, the fourth parameter the damping omega (4/3) instead of the over-correction
                nu = int(precond[1]) if len(precond) > 1 else 2
                ncs = int(precond[2]) if len(precond) > 2 else 16
                theta = float(precond[3]) if len(precond) > 3 else 0.08
                over = float(precond[4]) if len(precond) > 4 else (4.0 / 3.0 if smoothed else 1.0)
                shift = float(precond[5]) if len(precond) > 5 else 0.0
                rp = np.ascontiguousarray(op.csr[0], dtype=np.int32)
                ci = np.ascontiguousarray(op.csr[1], dtype=np.int32)
                va = np.ascontiguousarray(op.csr[2], dtype=dtype)
                set_amg = lib.primme_amd_operator_set_amg_smoothed if smoothed else lib.primme_amd_operator_set_amg
                rc = set_amg(self.oph, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                             va.ctypes.data_as(C.c_void_p), nu, ncs, theta, over, shift)
                if rc:
                    raise ValueError(f"precond={precond!r}: needs a real single-rank CSR operator ({rc}) with a positive diagonal, "
                                     f"steps >= 1, 0 <= theta < 1, {'0 < omega < 2' if smoothed else '1 <= over < 2'} and shift >= 0")
                lib.primme_amd_amg_stats(None, None, None)              # the counters are per process: start this solve at zero
                p.preconditioner = self.oph
                p.applyPreconditioner = C.cast(lib.primme_amd_amg_precond, C.c_void_p)
                p.correctionParams.precondition = 1
            elif amgh:
                # ("amg_hierarchy", H[, smooth_steps[, coarse_steps[, over]]]): the cycle of ("amg") / ("amg_smoothed") on a
                # hierarchy built once (AmgHierarchy); the smoother's parameters belong to this solve
                rc = lib.primme_amd_operator_set_amg_hierarchy(self.oph, H._handle(self), h_nu, h_ncs, h_over)
                if rc:
                    raise ValueError(f"precond=('amg_hierarchy', ...): the hierarchy does not fit this operator ({rc})")
                lib.primme_amd_amg_stats(None, None, None)              # the counters are per process: start this solve at zero
                p.preconditioner = self.oph
                p.applyPreconditioner = C.cast(lib.primme_amd_amg_precond, C.c_void_p)
                p.correctionParams.precondition = 1
            elif precond is not None:
                # "jacobi": per-vector shifts of the solver; ("jacobi", s): fixed K = diag(A) - s
                if precond == "jacobi": lib.primme_amd_operator_set_jacobi(self.oph, 0, 0.0)
                else: lib.primme_amd_operator_set_jacobi(self.oph, 1, float(precond[1]))
                p.preconditioner = self.oph
                p.applyPreconditioner = C.cast(lib.primme_amd_jacobi_precond, C.c_void_p)
                p.correctionParams.precondition = 1
            if self.comm is not None:
                p.commInfo = self.comm
                p.globalSumReal = C.cast(lib.primme_amd_global_sum, C.c_void_p)
            if profile:
                p.profile = b"phases"
            if self.be.device:
                import torch
                tdt = {"float64": torch.float64, "float32": torch.float32, "complex128": torch.complex128, "complex64": torch.complex64}[dtype.name]
                # (a zero-sized problem still gets a valid device pointer)
                evecs_buf = torch.zeros(max(ncols * nLocal, 1), dtype=tdt, device="cuda")
                evecs_t = evecs_buf[:ncols * nLocal].view(ncols, nLocal)
                if v0 is not None:
                    # the start vectors are uploaded once per Session and stay in HBM
                    key = (v0.shape, v0.dtype.str, hashlib.sha1(np.ascontiguousarray(v0).tobytes()).hexdigest())
                    if self._v0_cache is None or self._v0_cache[0] != key:
                        self._v0_cache = (key, torch.from_numpy(np.ascontiguousarray(v0.T)).to("cuda"))
                    evecs_t[nOC:nOC + initSize] = self._v0_cache[1]
                if cons is not None:
                    evecs_t[:nOC] = torch.from_numpy(np.ascontiguousarray(cons.T)).to("cuda")
                torch.cuda.synchronize()
                evecs_ptr = C.c_void_p(evecs_buf.data_ptr())
            else:
                evecs = np.zeros((ncols, nLocal), dtype=dtype)
                if cons is not None:
                    evecs[:nOC] = cons.T
                if v0 is not None:
                    evecs[nOC:nOC + initSize] = v0.T
                evecs_ptr = evecs.ctypes.data_as(C.c_void_p)
            solver = self.be.solver(dtype.name)

        if global_sum is not None:
            def gs(send, recv, count, pp, ierr):
                # operands arrive in the declared type: float for the single-precision entry points
                # unless the application set globalSumReal_type (reference primme_c.c:170-183)
                n_ = count[0]
                ct = C.c_float if pp[0].globalSumReal_type == F.primme_op_float else C.c_double
                a = np.ctypeslib.as_array(C.cast(send, C.POINTER(ct)), shape=(n_,)).astype(np.float64)
                np.ctypeslib.as_array(C.cast(recv, C.POINTER(ct)), shape=(n_,))[:] = global_sum(a)
                ierr[0] = 0
            gcb = F.GLOBAL_SUM(gs)
            keep.append(gcb)
            p.globalSumReal = C.cast(gcb, C.c_void_p)
        if monitor is not None:
            mcb = F.MONITOR(monitor)
            keep.append(mcb)
            p.monitorFun = C.cast(mcb, C.c_void_p)

        if lib.primme_set_method(m, C.byref(p)):
            raise ValueError("unknown method")
        if members:                      # {"dotted.name": value}: members by name through primme_set_member (members.py)
            apply_members(lib, p, members, keep)
        if tweak is not None:            # last word on the parameter structure (e.g. the correction equation's projectors)
            tweak(p)
        evals = np.zeros(numEvals, dtype=self.rdtype)
        resNorms = np.zeros(numEvals, dtype=self.rdtype)
        ret = solver(evals.ctypes.data_as(C.c_void_p), evecs_ptr, resNorms.ctypes.data_as(C.c_void_p), C.byref(p))
        if self.be.native_operator and self.be.device:
            import torch
            torch.cuda.synchronize()
            evecs = evecs_t.cpu().numpy() if return_evecs else None
        res = Result(ret, evals, None if evecs is None else evecs[nOC:nOC + numEvals].T.copy(), resNorms, p)
        if cheb:
            st = [C.c_long(0), C.c_long(0), C.c_long(0)]
            lib.primme_amd_chebyshev_stats(*[C.byref(v) for v in st])
            res.precond_stats = dict(zip(("applies", "operator_products", "fused_steps"), (v.value for v in st)))
        if mg:
            st = [C.c_long(0), C.c_long(0)]
            lib.primme_amd_multigrid_stats(*[C.byref(v) for v in st])
            res.precond_stats = dict(zip(("applies", "launches"), (v.value for v in st)))
        if amg or amgh:
            st = [C.c_long(0), C.c_long(0), C.c_long(0)]
            lib.primme_amd_amg_stats(*[C.byref(v) for v in st])
            res.precond_stats = dict(zip(("applies", "launches", "levels"), (v.value for v in st)))
        return res


_AMG_MAXLEVELS = 24


class _AmgLevel(C.Structure):
    _fields_ = [("n", C.c_int64), ("nnz", C.c_int64), ("nc", C.c_int64), ("rowptr", C.POINTER(C.c_int32)),
                ("colind", C.POINTER(C.c_int32)), ("values", C.POINTER(C.c_double)), ("dinv", C.POINTER(C.c_double)),
                ("rho", C.c_double), ("agg", C.POINTER(C.c_int32)), ("aggptr", C.POINTER(C.c_int32)),
                ("aggrows", C.POINTER(C.c_int32))]


class _AmgTransfer(C.Structure):
    _fields_ = [("pnnz", C.c_int64), ("prowptr", C.POINTER(C.c_int32)), ("pcolind", C.POINTER(C.c_int32)),
                ("pvalues", C.POINTER(C.c_double)), ("rrowptr", C.POINTER(C.c_int32)), ("rcolind", C.POINTER(C.c_int32)),
                ("rvalues", C.POINTER(C.c_double))]


class _AmgPlan(C.Structure):
    """primme_amd_amg_plan of include/primme_amd_io.h"""
    _fields_ = [("nlevels", C.c_int), ("shift", C.c_double), ("theta", C.c_double), ("level", _AmgLevel * _AMG_MAXLEVELS),
                ("omega", C.c_double), ("transfer", _AmgTransfer * _AMG_MAXLEVELS)]


def amg_download_plan(lib, handle):
    """primme_amd_amg_hierarchy_download for a hierarchy handle of the C ABI, as AmgHierarchy.plan() returns it"""
    P = C.POINTER(_AmgPlan)()
    download = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.POINTER(_AmgPlan)))(("primme_amd_amg_hierarchy_download", lib))
    free = C.CFUNCTYPE(None, C.POINTER(_AmgPlan))(("primme_amd_amg_plan_free", lib))
    rc = download(handle, C.byref(P))
    if rc:
        raise RuntimeError(f"primme_amd_amg_hierarchy_download failed: {rc}")

    def cp(p, n, dt):
        return np.ctypeslib.as_array(p, shape=(max(int(n), 1),))[:int(n)].astype(dt, copy=True)

    out = []
    for l in range(P.contents.nlevels):
        L, X = P.contents.level[l], P.contents.transfer[l]
        d = dict(n=int(L.n), nnz=int(L.nnz), nc=int(L.nc), rho=float(L.rho), dinv=cp(L.dinv, L.n, np.float64))
        if L.rowptr:
            d.update(rowptr=cp(L.rowptr, L.n + 1, np.int64), colind=cp(L.colind, L.nnz, np.int64), values=cp(L.values, L.nnz, np.float64))
        if L.nc > 0:
            d.update(agg=cp(L.agg, L.n, np.int64), aggptr=cp(L.aggptr, L.nc + 1, np.int64), aggrows=cp(L.aggrows, L.n, np.int64))
        if X.prowptr:
            d.update(pnnz=int(X.pnnz), prowptr=cp(X.prowptr, L.n + 1, np.int64), pcolind=cp(X.pcolind, X.pnnz, np.int64),
                     pvalues=cp(X.pvalues, X.pnnz, np.float64), rrowptr=cp(X.rrowptr, L.nc + 1, np.int64),
                     rcolind=cp(X.rcolind, X.pnnz, np.int64), rvalues=cp(X.rvalues, X.pnnz, np.float64))
        out.append(d)
    free(P)
    return out


class AmgHierarchy:
    """The hierarchy of the algebraic multigrid preconditioner as an object: built once, used by any number of solves through
    precond=("amg_hierarchy", H[, smooth_steps[, coarse_steps[, over]]]), on the Session it was built with or on another Session
    over the same matrix (a float32 one beside a float64 one, say).

    source: a Session (the hierarchy is built at once) or an Operator (it is built by the first solve that uses it).
    smoothed=True: smoothed aggregation with the damping omega (over must then be 1 in the solves); False: plain aggregation.
    setup="device": the prolongator, its transpose, the triple product, 1 / diag and the spectral bounds of every level are
    built on the device, the aggregation passes on the host (smoothed only); "host": everything on the host, the hierarchy of
    ("amg_smoothed") / ("amg") bit for bit.  close() releases the handle; a Session it is attached to keeps the device data
    alive until that Session is closed or given another preconditioner."""

    def __init__(self, source, smoothed=True, theta=0.08, omega=4.0 / 3.0, shift=0.0, setup="device"):
        if setup not in ("host", "device"):
            raise ValueError(f"setup={setup!r}: 'host' or 'device'")
        if setup == "device" and not smoothed:
            raise ValueError("setup='device' builds the smoothed hierarchy; plain aggregation has setup='host'")
        if not 0.0 <= theta < 1.0 or not shift >= 0.0 or (smoothed and not 0.0 < omega < 2.0):
            raise ValueError("needs 0 <= theta < 1, shift >= 0 and 0 < omega < 2")
        op = source.op if isinstance(source, Session) else source
        if not isinstance(op, Operator) or op.csr is None:
            raise ValueError("an AmgHierarchy is built from a Session or an Operator with CSR arrays")
        self.smoothed, self.theta, self.omega, self.shift, self.setup = bool(smoothed), float(theta), float(omega), float(shift), setup
        self.n, self.matrix_nnz = int(op.nrows), int(op.csr[0][-1])
        self.closed = False
        self._h, self._lib = None, None
        if isinstance(source, Session):
            self._handle(source)

    def _handle(self, session):
        """the library's handle, built with `session`'s operator when there is none yet"""
        if self.closed:
            raise ValueError("the AmgHierarchy is closed")
        if self._h is None:
            lib, op = session.lib, session.op
            if not (session.be.native_operator and hasattr(lib, "primme_amd_amg_hierarchy_create")):
                raise ValueError(f"an AmgHierarchy lives on the device of the product library; back end {session.backend!r} has none")
            if session.cplx or session.comm is not None or op.csr is None or (op.nrows, int(op.csr[0][-1])) != (self.n, self.matrix_nnz):
                raise ValueError("an AmgHierarchy is built with a real single-rank CSR operator, the one it was made for")
            rp = np.ascontiguousarray(op.csr[0], dtype=np.int32)
            ci = np.ascontiguousarray(op.csr[1], dtype=np.int32)
            va = np.ascontiguousarray(op.csr[2], dtype=session.dtype)
            h = C.c_void_p()
            rc = lib.primme_amd_amg_hierarchy_create(session.oph, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                                     va.ctypes.data_as(C.c_void_p), int(self.smoothed), self.theta, self.omega, self.shift,
                                                     1 if self.setup == "device" else 0, C.byref(h))
            if rc:
                raise ValueError(f"AmgHierarchy: the library refuses the matrix or the parameters ({rc}): it needs a symmetric matrix "
                                 "with a positive diagonal on every level")
            self._h, self._lib = h, lib
        return self._h

    def _info(self):
        if self._h is None:
            raise ValueError("the AmgHierarchy is closed" if self.closed else "the AmgHierarchy is not built yet: its first solve builds it")
        nl, att = C.c_int(0), C.c_long(0)
        rows, nnz, pnnz = ((C.c_int64 * _AMG_MAXLEVELS)() for _ in range(3))
        ss, ds = C.c_double(0), C.c_double(0)
        self._lib.primme_amd_amg_hierarchy_info(self._h, C.byref(nl), rows, nnz, pnnz, C.byref(ss), C.byref(ds), C.byref(att))
        fb = C.c_int(0)
        stages = (C.c_double * (_AMG_MAXLEVELS * 6))()
        self._lib.primme_amd_amg_hierarchy_stages(self._h, C.byref(fb), stages)
        k = nl.value
        return dict(levels=k, rows=list(rows[:k]), nnz=list(nnz[:k]), pnnz=list(pnnz[:k]), setup_seconds=ss.value, device_seconds=ds.value,
                    times_attached=att.value, fallback_levels=fb.value,
                    stage_seconds=[dict(zip(("aggregate", "prolongation", "transpose", "galerkin", "finish", "download"), stages[6 * l:6 * l + 6]))
                                   for l in range(max(k - 1, 0))])

    levels = property(lambda self: self._info()["levels"])
    rows = property(lambda self: self._info()["rows"])
    nnz = property(lambda self: self._info()["nnz"])
    setup_seconds = property(lambda self: self._info()["setup_seconds"])
    device_seconds = property(lambda self: self._info()["device_seconds"])
    fallback_levels = property(lambda self: self._info()["fallback_levels"])
    times_attached = property(lambda self: self._info()["times_attached"])
    stage_seconds = property(lambda self: self._info()["stage_seconds"])

    def plan(self):
        """the hierarchy read back from the device: a list of dicts per level (n, nnz, nc, rho, dinv; from level 1 on rowptr,
        colind, values; but on the last level agg, aggptr, aggrows and, smoothed, pnnz, prowptr, pcolind, pvalues, rrowptr,
        rcolind, rvalues) as numpy arrays.  Level 0 has no matrix: it is the operator's."""
        self._info()
        return amg_download_plan(self._lib, self._h)

    def close(self):
        if self._h is not None:
            self._lib.primme_amd_amg_hierarchy_destroy(self._h)
        self._h, self.closed = None, True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def eigsh(op, backend="hip", comm=None, dtype=np.float64, complex_form="native", mass=None, **kw):
    """One-shot: compute a few eigenpairs of the symmetric operator `op` (see Session.solve).

    v0: optional (nLocal x initSize) initial guesses -> initBasisMode defaults to
    primme_init_user so that no random numbers enter (parity runs).
    precond: None | "jacobi" (Davidson: per-vector shifts) | ("jacobi", shift) (fixed shift) |
    ("chebyshev", steps, lo[, hi]) (polynomial preconditioner with the solver's shifts; hi defaults to the Gershgorin
    bound) | ("chebyshev", steps, lo, hi, shift) (fixed shift).  Result.precond_stats then holds its counters.
    ("multigrid", dims[, smooth_steps[, coarse_steps[, scale[, shift]]]]): one geometric multigrid V-cycle for
    scale * Laplacian + shift on the grid dims = (nx[, ny[, nz]]), x fastest (defaults 2, 16, 1, 0), for grid Laplacians in any
    operator form and for -Laplacian + V with shift about the mean of V; Result.precond_stats = {"applies", "launches"}.
    ("amg"[, smooth_steps[, coarse_steps[, theta[, over[, shift]]]]]): one aggregation algebraic multigrid V-cycle for A + shift
    on a hierarchy built from the CSR arrays of the operator, a symmetric matrix with a positive diagonal (defaults 2, 16, 0.08,
    1, 0): FEM, structural and graph matrices without a grid; Result.precond_stats = {"applies", "launches", "levels"}.
    ("amg_smoothed"[, smooth_steps[, coarse_steps[, theta[, omega[, shift]]]]]): the same cycle on the hierarchy of smoothed
    aggregation, P = (I - (omega / rho) D^-1 M) T (defaults 2, 16, 0.08, 4/3, 0): iteration counts that grow far less with the
    problem size, for a costlier host set-up and denser coarse levels; the same precond_stats.
    members: {"name": value} set through primme_set_member after the method preset and before `tweak`, e.g.
    {"correctionParams.maxInnerIterations": 0, "projectionParams.projection": "primme_proj_refined"}; a string for an
    enum member is an enumerator name (primme_constant_info); an unknown member or enumerator is a ValueError.
    """
    s = Session(op, comm=comm, dtype=dtype, backend=backend, complex_form=complex_form, mass=mass)
    try:
        return s.solve(**kw)
    finally:
        s.close()
