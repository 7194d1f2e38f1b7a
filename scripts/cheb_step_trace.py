"""One Chebyshev step, fused against generic, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python scripts/cheb_step_trace.py --case lap --cols 8

runs --reps (default 20) fused steps (hipk_csr_cheb_step) and as many generic ones (hipk_csr_matvec into a scratch panel +
hipk_cheb_update) on the same panels, after 3 warm-up rounds of each.  The fused kernels are the <..., true> instantiations of
the product kernels, the generic pair is the <..., false> product kernel and cheb_update_kernel, so the per-name averages of
NAME_kernel_stats.csv give both sides: time of a step = (sum over its kernels of calls x average) / (reps + 3).

Cases: lap = 5-point Laplacian 3162 x 3163 (row-pattern form), lunda = LUNDA.mtx tiled 34 014 x (CSR row tiles).  Prints the
operator form in use (hipk_csr_format) and the bytes each side moves per step."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from primme_amd import _ffi as F  # noqa: E402
from primme_amd import problems  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("lap", "lunda"), required=True)
    ap.add_argument("--cols", type=int, required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    import torch
    lib = F.load_product()
    if a.case == "lap":
        rp, ci, va, n = problems.laplacian_csr((316, 317) if a.small else (3162, 3163))
    else:
        from cheb_headline import lunda_tiled
        rp, ci, va, n, _ = lunda_tiled(340 if a.small else 34014)
    rp = np.ascontiguousarray(rp, dtype=np.int32); ci = np.ascontiguousarray(ci, dtype=np.int32); va = np.ascontiguousarray(va, dtype=np.float64)
    ctx, Ah = C.c_void_p(), C.c_void_p()
    assert lib.hipk_ctx_create(C.byref(ctx), None) == 0
    assert lib.hipk_csr_create(ctx, F.HIPK_F64, n, n, 0, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p), va.ctypes.data_as(C.c_void_p), C.byref(Ah)) == 0
    st = lib.hipk_ctx_stream(ctx)
    nb, ld = a.cols, (n + 15) // 16 * 16 + 16
    X, Y0, Y1, W = (torch.randn((nb, ld), dtype=torch.float64, device="cuda") for _ in range(4))
    torch.cuda.synchronize()
    cf = F.HipkChebCoef()
    for c in range(nb):
        cf.cy[c], cf.cp[c], cf.cx[c], cf.cw[c] = 0.9 + 0.01 * c, -0.3, 0.05, -0.05      # a contraction: the iterates stay bounded
    P = lambda t: C.c_void_p(t.data_ptr())
    Y = [Y0, Y1]
    for r in range(a.reps + 3):
        k, p = r % 2, (r + 1) % 2
        assert lib.hipk_csr_cheb_step(Ah, st, nb, C.byref(cf), P(X), ld, P(Y[k]), ld, P(Y[p]), ld, P(Y[p]), ld) == 0
    assert lib.hipk_sync(ctx) == 0
    for r in range(a.reps + 3):
        k, p = r % 2, (r + 1) % 2
        assert lib.hipk_csr_matvec(Ah, st, P(Y[k]), ld, P(W), ld, nb) == 0
        assert lib.hipk_cheb_update(st, F.HIPK_F64, n, nb, C.byref(cf), P(X), ld, P(W), ld, P(Y[k]), ld, P(Y[p]), ld, P(Y[p]), ld) == 0
    assert lib.hipk_sync(ctx) == 0
    fmt = lib.hipk_csr_format(Ah)
    nnz = len(va)
    vec = 8.0 * n * nb
    print(json.dumps(dict(case=a.case, cols=nb, n=n, nnz=nnz, format=fmt, rounds=a.reps + 3, finite=bool(torch.isfinite(Y[0]).all().item()),
                          vector_bytes_fused=4 * vec, vector_bytes_generic=7 * vec, csr_matrix_bytes=12.0 * nnz + 4.0 * n)), flush=True)
    lib.hipk_csr_destroy(Ah); lib.hipk_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
