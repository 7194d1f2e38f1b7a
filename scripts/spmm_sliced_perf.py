"""The sliced-ELL form (HIPK_CSR_SLICED, csrc/hipk_sparse_sell.hip) against the CSR row tiles on the LUNDA tiling of BASELINE
configs[2] (tests/golden/reference_driver/LUNDA.mtx through primme_amd.ingest: mm_read + tile_block_diagonal, as bench.py builds
it): hipk_csr_matvec for 1 and 8 columns, both forms on the SAME handle in the SAME process, switched with hipk_set_spmv_format
and alternated batch by batch (boxes differ by a few per cent: only this comparison counts).  Device events around batches of
`reps` launches; the median of `samples` batches and their spread are reported.  The vectors rotate over panels larger than the
Infinity Cache.  Also checks that the two forms agree to rounding at this size.

Then, with --solves, one configs[2] solve each way through scripts/config3_run.py in fresh processes (HIPK_SPMV_SELL=1 / unset).

usage: python scripts/spmm_sliced_perf.py [--tiles 34014] [--reps 20] [--samples 7] [--solves] [--out profiles/sliced_spmm.json]"""
import argparse, ctypes as C, json, os, subprocess, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12        # HBM3E bytes per second (MI355X)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tiles", type=int, default=34014)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--samples", type=int, default=7)
    ap.add_argument("--solves", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sliced_spmm.json"))
    args = ap.parse_args()
    import torch
    from primme_amd import _ffi as F, ingest
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it has no CPU path")
    lib = F.load_product()
    rp0, ci0, va0, n0, _ = ingest.mm_read(lib, os.path.join(ROOT, "tests", "golden", "reference_driver", "LUNDA.mtx"))
    T = args.tiles
    rp, ci, va = ingest.tile_block_diagonal(lib, rp0, ci0, va0, T, 1.0, 1.0 / T)
    n, nnz = n0 * T, len(va)
    ctx = C.c_void_p(); assert lib.hipk_ctx_create(C.byref(ctx), None) == 0
    A = C.c_void_p()
    assert lib.hipk_csr_create_opts(ctx, F.HIPK_F64, n, n, 0, rp.ctypes.data_as(C.c_void_p), ci.ctypes.data_as(C.c_void_p),
                                    va.ctypes.data_as(C.c_void_p), F.HIPK_CSR_SLICED, C.byref(A)) == 0
    assert lib.hipk_csr_sliced(A) == 1, "the sliced form was not built"
    lib.hipk_csr_index_bytes.argtypes = [C.c_void_p]
    out = dict(workload=f"LUNDA.mtx tiled block-diagonally {T} x: n = {n}, nnz = {nnz}, float64", x_gather="global memory (L2); no LDS window",
               padding_ratio=lib.hipk_csr_sliced_padding(A), reps=args.reps, samples=args.samples, widths={})
    print(f"n = {n}, nnz = {nnz}, padded / nnz = {out['padding_ratio']:.4f}", flush=True)

    def batch(fn):
        ms = C.c_float()
        lib.hipk_timer_start(ctx)
        for _ in range(args.reps): fn()
        lib.hipk_timer_stop(ctx, C.byref(ms))
        return 1e3 * ms.value / args.reps

    for ncols in (1, 8):
        npan = max(2, int(1.2e9 // (8 * n * ncols)))                   # > 1 GB of input panels: nothing of x survives in the Infinity Cache
        X = torch.randn((npan, ncols, n), dtype=torch.float64, device="cuda")
        Y = torch.zeros((npan, ncols, n), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        it = [0]

        def product():
            p = it[0] % npan; it[0] += 1
            lib.hipk_csr_matvec(A, None, X[p].data_ptr(), n, Y[p].data_ptr(), n, ncols)
        us = {1: [], 0: []}
        res = {}
        for fmt in (1, 0):                                             # warm-up of both forms, and their results on panel 0
            lib.hipk_set_spmv_format(fmt)
            it[0] = 0
            for _ in range(3): product()
            lib.hipk_sync(ctx); torch.cuda.synchronize()
            res[fmt] = Y[0].cpu().numpy().copy()
        for _ in range(args.samples):                                  # alternate the forms batch by batch
            for fmt in (1, 0):
                lib.hipk_set_spmv_format(fmt)
                us[fmt].append(batch(product))
        lib.hipk_set_spmv_format(1)
        es = 8
        bytes_ = {1: lib.hipk_csr_product_bytes(A, 0) + 2.0 * n * es * (ncols - 1),
                  0: nnz * (es + lib.hipk_csr_index_bytes(A)) + (n + 1) * 4.0 + 2.0 * n * es * ncols}
        scale = float(np.max(np.abs(res[0])))
        row = dict(max_abs_difference_over_max_abs_y=float(np.max(np.abs(res[1] - res[0])) / scale))
        for fmt, label in ((1, "sliced"), (0, "row_tiles")):
            med = float(np.median(us[fmt]))
            row[label] = dict(us_median=round(med, 1), us_min=round(min(us[fmt]), 1), us_max=round(max(us[fmt]), 1),
                              streamed_bytes=bytes_[fmt], fraction_of_8TBps=round(bytes_[fmt] / (med * 1e-6) / PEAK, 4))
        row["row_tiles_over_sliced"] = round(row["row_tiles"]["us_median"] / row["sliced"]["us_median"], 4)
        out["widths"][str(ncols)] = row
        print(ncols, json.dumps(row), flush=True)
        del X, Y
        torch.cuda.empty_cache()
    lib.hipk_csr_destroy(A)
    lib.hipk_ctx_destroy(ctx)

    if args.solves:
        out["configs2_solve"] = {}
        for label, val in (("sliced", "1"), ("row_tiles", None)):
            env = dict(os.environ)
            env.pop("HIPK_SPMV_SELL", None)
            if val: env["HIPK_SPMV_SELL"] = val
            r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "config3_run.py"), "--tiles", str(T), "--prof", "--reps", "2"],
                               env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode or not line:
                raise SystemExit(f"config3_run.py ({label}) failed:\n{r.stdout[-3000:]}")
            out["configs2_solve"][label] = json.loads(line[-1])
            print(label, line[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
