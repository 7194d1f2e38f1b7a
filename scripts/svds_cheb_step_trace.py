"""One Chebyshev step of the singular value preconditioner on A', one-pass against generic, for a kernel trace of its own:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o NAME -- python scripts/svds_cheb_step_trace.py --case band --cols 8

runs --reps (default 20) one-pass steps (hipk_csr_cheb_step_gather on A' with G = z) and as many generic ones (hipk_csr_matvec of
A' into a product panel + hipk_cheb_update) on the same panels, after 3 warm-up rounds of each.  The product z = A y_k that both
sides need first is not part of either.  The one-pass kernel is the <..., true> instantiation of the windowed block kernel, the
generic pair is the plain product kernel and cheb_update_kernel, so the per-name averages of NAME_kernel_stats.csv give both sides.

Cases: band = a banded rectangular matrix, 4 000 000 x 3 000 000, 3 entries per row (A' has 4 per row);
config4 = problems.svds_synthetic_csr(8e6, 2e6), the matrix of BASELINE configs[4].  Prints hipk_csr_format of A': only the
row-tile form (0) has a one-pass step — for any other the script says so and times the generic pair alone."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from primme_amd import _ffi as F  # noqa: E402
from primme_amd import problems  # noqa: E402
from primme_amd.svds_api import transpose_csr  # noqa: E402


def band(m, n):
    i = np.arange(m, dtype=np.int64)
    c0 = np.minimum((i * n) // m, n - 3)
    ci = np.stack([c0, c0 + 1, c0 + 2], axis=1).reshape(-1).astype(np.int32)
    va = (1.0 + ((np.arange(3 * m) % 7) / 7.0)) * np.where(np.arange(3 * m) % 3 == 1, -1.0, 1.0)
    return np.arange(0, 3 * m + 1, 3, dtype=np.int32), ci, va


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("band", "config4"), required=True)
    ap.add_argument("--cols", type=int, required=True)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    import torch
    lib = F.load_product()
    if a.case == "band":
        m, n = (40000, 30000) if a.small else (4000000, 3000000)
        rp, ci, va = band(m, n)
    else:
        m, n = (80000, 20000) if a.small else (8000000, 2000000)
        rp, ci, va = problems.svds_synthetic_csr(m, n)
    rpT, ciT, vaT = transpose_csr(m, n, rp, ci, va)
    rpT = np.ascontiguousarray(rpT, dtype=np.int32); ciT = np.ascontiguousarray(ciT, dtype=np.int32); vaT = np.ascontiguousarray(vaT, dtype=np.float64)
    ctx, At = C.c_void_p(), C.c_void_p()
    assert lib.hipk_ctx_create(C.byref(ctx), None) == 0
    assert lib.hipk_csr_create_rect(ctx, F.HIPK_F64, n, m, rpT.ctypes.data_as(C.c_void_p), ciT.ctypes.data_as(C.c_void_p), vaT.ctypes.data_as(C.c_void_p),
                                    C.byref(At)) == 0
    lib.hipk_csr_format.argtypes = [C.c_void_p]
    fmt = lib.hipk_csr_format(At)
    st = lib.hipk_ctx_stream(ctx)
    nb, ldn, ldm = a.cols, (n + 15) // 16 * 16 + 16, (m + 15) // 16 * 16 + 16
    X, Y0, Y1, W = (torch.randn((nb, ldn), dtype=torch.float64, device="cuda") for _ in range(4))
    G = torch.randn((nb, ldm), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    cf = F.HipkChebCoef()
    for c in range(nb):
        cf.cy[c], cf.cp[c], cf.cx[c], cf.cw[c] = 0.6 + 0.01 * c, -0.3, 0.05, -0.01       # a contraction: the iterates stay bounded
    P = lambda t: C.c_void_p(t.data_ptr())
    Y = [Y0, Y1]
    fused_rc = None
    for r in range(a.reps + 3):
        k, p = r % 2, (r + 1) % 2
        fused_rc = lib.hipk_csr_cheb_step_gather(At, st, nb, C.byref(cf), P(X), ldn, P(G), ldm, P(Y[k]), ldn, P(Y[p]), ldn, P(Y[p]), ldn)
        assert fused_rc == (0 if fmt == 0 else 1), fused_rc
        if fused_rc:
            break
    assert lib.hipk_sync(ctx) == 0
    for r in range(a.reps + 3):
        k, p = r % 2, (r + 1) % 2
        assert lib.hipk_csr_matvec(At, st, P(G), ldm, P(W), ldn, nb) == 0
        assert lib.hipk_cheb_update(st, F.HIPK_F64, n, nb, C.byref(cf), P(X), ldn, P(W), ldn, P(Y[k]), ldn, P(Y[p]), ldn, P(Y[p]), ldn) == 0
    assert lib.hipk_sync(ctx) == 0
    nnz = len(vaT)
    vec_n, vec_m = 8.0 * n * nb, 8.0 * m * nb
    print(json.dumps(dict(case=a.case, cols=nb, rows_of_At=n, cols_of_At=m, nnz=nnz, format=fmt, one_pass_available=fused_rc == 0, rounds=a.reps + 3,
                          finite=bool(torch.isfinite(Y[0]).all().item()), vector_bytes_one_pass=4 * vec_n + vec_m,
                          vector_bytes_generic=(1 + 5) * vec_n + vec_m, csr_matrix_bytes=12.0 * nnz + 4.0 * n)), flush=True)
    lib.hipk_csr_destroy(At); lib.hipk_ctx_destroy(ctx)


if __name__ == "__main__":
    main()
