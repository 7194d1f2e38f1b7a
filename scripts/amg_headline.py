"""Timed solves with the aggregation algebraic multigrid preconditioner against the other preconditioners; ONE configuration
per invocation, so that a job runs each under a time limit of its own and chains them:

    python scripts/amg_headline.py --case lunda --config jacobi       # configs[2]'s problem as bench.py defines it
    python scripts/amg_headline.py --case lunda --config amg
    python scripts/amg_headline.py --case lap   --config none         # the base: first, the Chebyshev row reads its eigenvalues
    python scripts/amg_headline.py --case lap   --config chebyshev
    python scripts/amg_headline.py --case lap   --config multigrid
    python scripts/amg_headline.py --case lap   --config amg
    python scripts/amg_headline.py --case lap   --config amg_smoothed # smoothed aggregation; also for --case lunda
    python scripts/amg_headline.py --case lap   --config amg_hierarchy # one hierarchy built on the device, two solves on it (4q);
                                                                      # also for --case lunda

Every invocation adds (or replaces) its row in profiles/amg_headline.json (--out): the seconds of each of --repeats solves
after a short warm-up solve of the same configuration, their median, outer iterations, matvecs, the preconditioner's counters
and the largest eigenvalue error against the truth.  The amg rows also hold the set-up seconds on the host (one call of
primme_amd_amg_plan_create or _create_smoothed on the same arrays, timed by itself), the rows of the levels and the operator
complexity sum nnz(M_l) / nnz(M_0).

Cases
  lunda  BASELINE configs[2]: LUNDA.mtx tiled block-diagonally 34 014 times (tile t scaled by 1 + t/T, n = 5 000 058), 20
         eigenvalues closest to 4.4764e8, JDQMR, block size 8, eps 1e-8 |A|; Jacobi is K = diag(A) - shift as in bench.py
  lap    the headline problem: CSR 5-point Laplacian 3162 x 3163, 10 smallest, GD+k, block 1, eps 1e-8 |A|, |A| = 8
  --small shrinks both (340 tiles; 316 x 317): a functional check.  --max-outer caps the outer iterations of every solve."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from primme_amd import ingest as ingest_c  # noqa: E402
from primme_amd import problems  # noqa: E402
from primme_amd.api import Operator, Session  # noqa: E402


class Level(C.Structure):
    _fields_ = [("n", C.c_int64), ("nnz", C.c_int64), ("nc", C.c_int64), ("rowptr", C.c_void_p), ("colind", C.c_void_p),
                ("values", C.c_void_p), ("dinv", C.c_void_p), ("rho", C.c_double), ("agg", C.c_void_p), ("aggptr", C.c_void_p),
                ("aggrows", C.c_void_p)]


class Plan(C.Structure):
    _fields_ = [("nlevels", C.c_int), ("shift", C.c_double), ("theta", C.c_double), ("level", Level * 24)]


def host_setup(lib, rp, ci, va, shift=0.0, theta=0.08, omega=None):
    """(seconds of primme_amd_amg_plan_create, or of _create_smoothed with omega, rows per level, operator complexity)"""
    lib.primme_amd_amg_plan_create_smoothed.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double,
                                                        C.c_double, C.POINTER(C.POINTER(Plan))]
    lib.primme_amd_amg_plan_create.argtypes = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_double, C.c_double,
                                               C.POINTER(C.POINTER(Plan))]
    lib.primme_amd_amg_plan_free.argtypes = [C.POINTER(Plan)]
    rp, ci, va = (np.ascontiguousarray(a, dtype=t) for a, t in ((rp, np.int32), (ci, np.int32), (va, np.float64)))
    P = C.POINTER(Plan)()
    t0 = time.perf_counter()
    if omega is None:
        rc = lib.primme_amd_amg_plan_create(len(rp) - 1, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 8, shift, theta, C.byref(P))
    else:
        rc = lib.primme_amd_amg_plan_create_smoothed(len(rp) - 1, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, 8, shift, theta, omega, C.byref(P))
    secs = time.perf_counter() - t0
    assert rc == 0, rc
    lv = [P.contents.level[l] for l in range(P.contents.nlevels)]
    rows, cx = [int(v.n) for v in lv], sum(int(v.nnz) for v in lv) / int(lv[0].nnz)
    lib.primme_amd_amg_plan_free(P)
    return secs, rows, cx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("lunda", "lap"), required=True)
    ap.add_argument("--config", choices=("none", "jacobi", "chebyshev", "multigrid", "amg", "amg_smoothed", "amg_hierarchy"), required=True)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--max-outer", type=int, default=60000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "amg_headline.json"))
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    from primme_amd import _ffi as F
    lib = F.load_product()
    if a.case == "lunda":
        mtx = os.path.join(ROOT, "tests", "golden", "reference_driver", "LUNDA.mtx")
        rp0, ci0, va0, n0, _ = ingest_c.mm_read(lib, mtx)
        T, shift = (340 if a.small else 34014), 4.4764e8
        rp, ci, va = ingest_c.tile_block_diagonal(lib, rp0, ci0, va0, T, 1.0, 1.0 / T)
        n = n0 * T
        A0 = np.zeros((n0, n0)); A0[np.repeat(np.arange(n0), np.diff(rp0)), ci0] = va0
        w = (np.linalg.eigvalsh(A0)[None, :] * (1.0 + np.arange(T) / T)[:, None]).ravel()
        aN = float(np.abs(w).max())
        exact = np.sort(w[np.argsort(np.abs(w - shift))][:20])
        kw = dict(numEvals=20, target="closest_abs", targetShifts=[shift], method="JDQMR", maxBlockSize=8, eps=1e-8, aNorm=aN,
                  return_evecs=False)
        workload = f"configs[2]: LUNDA.mtx tiled {T}x (n = {n}), 20 eigenvalues closest to {shift:.4e}, JDQMR, block 8, eps 1e-8 |A|"
        allowed = {"jacobi": ("jacobi K = diag(A) - shift", ("jacobi", shift)), "amg": ("amg V(2,2)", ("amg",)),
                   "amg_smoothed": ("amg smoothed V(2,2)", ("amg_smoothed",))}
    else:
        dims, aN = ((316, 317) if a.small else (3162, 3163)), 8.0
        rp, ci, va, n = problems.laplacian_csr(dims)
        exact = problems.laplacian_eigenvalues(dims, 10)
        kw = dict(numEvals=10, target="smallest", method="GD_plusK", eps=1e-8, aNorm=aN, v0=problems.start_vector(n), return_evecs=False)
        workload = f"CSR 5-point Laplacian {dims[0]} x {dims[1]}, 10 smallest, GD+k, block 1, eps 1e-8 |A|"
        allowed = {"none": ("none", None), "chebyshev": ("chebyshev steps=16", "chebyshev"), "multigrid": ("multigrid V(2,2)", ("multigrid", dims, 2, 16)),
                   "amg": ("amg V(2,2)", ("amg",)), "amg_smoothed": ("amg smoothed V(2,2)", ("amg_smoothed",))}
    allowed["amg_hierarchy"] = ("amg hierarchy, device set-up, V(2,2)", ("amg_hierarchy",))
    if a.config not in allowed:
        raise SystemExit(f"case {a.case} has the configurations {sorted(allowed)}")
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rows = doc.setdefault(a.case + ("_small" if a.small else ""), dict(workload=workload, rows=[]))["rows"]
    label, precond = allowed[a.config]
    if precond == "chebyshev":
        base = [r for r in rows if r["label"] == "none"]
        if not base:
            raise SystemExit(f"{a.out} has no 'none' row for case {a.case}: run --config none first")
        th = np.sort(np.array(base[0]["evals"]))
        precond = ("chebyshev", 16, float(th[-1] + (th[-1] - th[0]) / 10))
    row = dict(label=label, precond=[list(v) if isinstance(v, tuple) else v for v in precond] if isinstance(precond, tuple) else precond,
               command=" ".join(["python", "scripts/amg_headline.py"] + sys.argv[1:]))
    if a.config in ("amg", "amg_smoothed"):
        secs, lrows, cx = host_setup(lib, rp, ci, va, omega=4.0 / 3.0 if a.config == "amg_smoothed" else None)
        row.update(setup_seconds_host=secs, level_rows=lrows, levels=len(lrows), operator_complexity=cx)
        print(json.dumps(row), flush=True)
    kw["maxOuterIterations"] = a.max_outer
    if a.config == "amg_hierarchy":
        # the host set-up by itself, then per repeat ONE hierarchy built on the device (whole call, device stages,
        # per stage and level; the host's remainder is the aggregate and download lines) and two solves on it; to be read against
        # the "amg smoothed V(2,2)" row, whose every solve includes the host set-up and the upload
        from primme_amd.api import AmgHierarchy
        secs, lrows, cx = host_setup(lib, rp, ci, va, omega=4.0 / 3.0)
        row.update(setup_seconds_host=secs, level_rows_host=lrows)
        s = Session(Operator(n, csr=(rp, ci, va)))
        # the host's stages per level: the same build with every level sent to the host routines (entry limit 0); the lines are
        # P with its transpose, the triple product, the finish, and the upload in the place of the download
        os.environ["PRIMME_AMD_AMG_SETUP_MAX_ENTRIES"] = "0"
        Hh = AmgHierarchy(s, setup="device")
        del os.environ["PRIMME_AMD_AMG_SETUP_MAX_ENTRIES"]
        assert Hh.fallback_levels == Hh.levels - 1
        row.update(host_route_per_level=dict(setup_seconds=Hh.setup_seconds, level_rows=Hh.rows, level_nnz=Hh.nnz, stage_seconds=Hh.stage_seconds))
        Hh.close()
        print(json.dumps(row), flush=True)
        builds, first, second = [], [], []
        for _ in range(a.repeats):
            H = AmgHierarchy(s, setup="device")
            builds.append(dict(setup_seconds=H.setup_seconds, device_seconds=H.device_seconds, fallback_levels=H.fallback_levels,
                               level_rows=H.rows, level_nnz=H.nnz, stage_seconds=H.stage_seconds))
            for out in (first, second):
                t0 = time.perf_counter()
                r = s.solve(precond=("amg_hierarchy", H), **kw)
                out.append(time.perf_counter() - t0)
            H.close()
        s.close()
        ev = np.sort(r.evals)
        med = sorted(builds, key=lambda b: b["setup_seconds"])[len(builds) // 2]
        row.update(ret=r.ret, converged_pairs=int(r.initSize), builds=builds, setup_seconds_device_route_median=med["setup_seconds"],
                   device_stage_seconds_median_build=med["device_seconds"],
                   host_remainder_seconds_median_build=dict(aggregate=sum(x["aggregate"] for x in med["stage_seconds"]),
                                                            download=sum(x["download"] for x in med["stage_seconds"])),
                   seconds_first_solve=first, seconds_second_solve=second, seconds_first_solve_median=float(np.median(first)),
                   seconds_second_solve_median=float(np.median(second)), outer_iterations=r.stats["numOuterIterations"],
                   matvecs=r.stats["numMatvecs"], precond_stats=r.precond_stats,
                   max_eval_error_vs_truth=float(np.max(np.abs(ev - exact[:len(ev)]))) if r.ret == 0 else None, evals=ev.tolist())
        rows[:] = [x for x in rows if x["label"] != label] + [row]
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        json.dump(doc, open(a.out, "w"), indent=1)
        print(json.dumps({k: v for k, v in row.items() if k not in ("evals", "builds")}), flush=True)
        return
    s = Session(Operator(n, csr=(rp, ci, va)))
    s.solve(precond=precond, **dict(kw, maxOuterIterations=min(20, a.max_outer)))      # warm-up, not timed
    secs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        r = s.solve(precond=precond, **kw)              # returns after the device has finished; amg: set-up and upload included
        secs.append(time.perf_counter() - t0)
    s.close()
    ev = np.sort(r.evals)
    row.update(ret=r.ret, converged_pairs=int(r.initSize), seconds=secs, seconds_median=float(np.median(secs)),
               outer_iterations=r.stats["numOuterIterations"], matvecs=r.stats["numMatvecs"], precond_stats=r.precond_stats,
               max_eval_error_vs_truth=float(np.max(np.abs(ev - exact[:len(ev)]))) if r.ret == 0 else None, evals=ev.tolist())
    rows[:] = [x for x in rows if x["label"] != label] + [row]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in row.items() if k != "evals"}), flush=True)


if __name__ == "__main__":
    main()
