"""Timed solves with and without the Chebyshev polynomial preconditioner; ONE configuration per invocation, so that a job runs
each under a time limit of its own and chains them:

    python scripts/cheb_headline.py --case lap   --config none          # the base: always first, the others read its row
    python scripts/cheb_headline.py --case lap   --config 8             # steps = 8
    python scripts/cheb_headline.py --case lunda --config none  ...

Every invocation adds (or replaces) its row in profiles/cheb_headline.json (--out).  A row holds the seconds of each of
--repeats solves (default 3) after a 50-iteration warm-up solve of the same configuration (allocations, first launches, the Gershgorin
pass of set_chebyshev's first call), their median, outer iterations, matvecs, operator products inside the preconditioner and
the largest eigenvalue error against the known spectrum.  The comparison base of a case is its `none` row of the same file.

Cases
  lap    the headline problem: 5-point Laplacian 3162 x 3163 (lap2d_10m), 10 smallest, GD+k, block 1, eps 1e-8 |A|, |A| = 8.
  lunda  the Matrix-Market tiling of bench.py's configs[2]: LUNDA.mtx tiled block-diagonally 34 014 times (n = 5 000 058),
         tile t scaled by 1 + t/T; 10 largest, GD+k, block 1, eps 1e-8 |A|.  (configs[2] itself targets interior eigenvalues,
         where no shift lies outside an interval that holds the rest of the spectrum; the largest end is the extremal problem
         of the same operator.)
  --small shrinks both (316 x 317; 340 tiles): a functional check.

Rule for the interval (no knowledge of the spectrum beyond the base solve): with theta_1 <= ... <= theta_k the wanted
eigenvalues the base solve returned and g = (theta_k - theta_1)/k their mean spacing,
  smallest: lo = theta_k + g, hi = the operator's Gershgorin upper bound (left to the library);
  largest:  hi = theta_1 - g, lo = the operator's Gershgorin lower bound (primme_amd_operator_gershgorin)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from primme_amd import _ffi as F  # noqa: E402
from primme_amd import problems  # noqa: E402
from primme_amd.api import Operator, Session  # noqa: E402


def lunda_tiled(T):
    from primme_amd import ingest
    lib = F.load_product()
    rp0, ci0, va0, n0, _ = ingest.mm_read(lib, os.path.join(ROOT, "tests", "golden", "reference_driver", "LUNDA.mtx"))
    rp, ci, va = ingest.tile_block_diagonal(lib, rp0, ci0, va0, T, 1.0, 1.0 / T)
    A0 = np.zeros((n0, n0)); A0[np.repeat(np.arange(n0), np.diff(rp0)), ci0] = va0
    w = np.sort((np.linalg.eigvalsh(A0)[None, :] * (1.0 + np.arange(T) / T)[:, None]).ravel())
    return rp, ci, va, n0 * T, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("lap", "lunda"), required=True)
    ap.add_argument("--config", required=True, help="none, or the number of steps")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cheb_headline.json"))
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    nev = 10
    if a.case == "lap":
        dims = (316, 317) if a.small else (3162, 3163)
        rp, ci, va, n = problems.laplacian_csr(dims)
        exact, aN, target = problems.laplacian_eigenvalues(dims, nev), 8.0, "smallest"
        workload = f"5-point Laplacian {dims[0]} x {dims[1]}, {nev} smallest, GD+k, eps 1e-8 |A|"
    else:
        T = 340 if a.small else 34014
        rp, ci, va, n, w = lunda_tiled(T)
        exact, aN, target = w[-nev:], float(np.abs(w).max()), "largest"
        workload = f"LUNDA.mtx tiled block-diagonally {T} x (n = {n}), {nev} largest, GD+k, eps 1e-8 |A|"
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rows = doc.setdefault(a.case, dict(workload=workload, rows=[]))["rows"]
    s = Session(Operator(n, csr=(rp, ci, va)))
    kw = dict(numEvals=nev, target=target, method="GD_plusK", eps=1e-8, aNorm=aN, v0=problems.start_vector(n), return_evecs=False,
              maxOuterIterations=60000)
    if a.config == "none":
        label, precond = "none", None
    else:
        base = [r for r in rows if r["label"] == "none"]
        if not base:
            raise SystemExit(f"{a.out} has no 'none' row for case {a.case}: run --config none first")
        th = np.sort(np.array(base[0]["evals"]))
        g = (th[-1] - th[0]) / nev
        if target == "smallest":
            precond = ("chebyshev", int(a.config), float(th[-1] + g))
        else:
            glo, ghi = C.c_double(), C.c_double()
            assert s.lib.primme_amd_operator_gershgorin(s.oph, C.byref(glo), C.byref(ghi)) == 0
            precond = ("chebyshev", int(a.config), glo.value, float(th[0] - g))
        label = f"chebyshev steps={a.config}"
    s.solve(precond=precond, **dict(kw, maxOuterIterations=50))      # warm-up, not timed
    secs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        r = s.solve(precond=precond, **kw)              # returns after the device has finished (the results are on the host)
        secs.append(time.perf_counter() - t0)
    st = r.precond_stats or dict(applies=0, operator_products=0, fused_steps=0)
    row = dict(label=label, precond=list(precond) if precond else None, ret=r.ret, seconds=secs, seconds_median=float(np.median(secs)),
               outer_iterations=r.stats["numOuterIterations"], matvecs=r.stats["numMatvecs"],
               operator_products_in_precond=st["operator_products"], fused_steps=st["fused_steps"],
               max_eval_error_vs_truth=float(np.max(np.abs(np.sort(r.evals) - exact))), evals=np.sort(r.evals).tolist())
    s.close()
    rows[:] = [x for x in rows if x["label"] != label] + [row]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in row.items() if k != "evals"}), flush=True)


if __name__ == "__main__":
    main()
