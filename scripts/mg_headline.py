"""Timed solves without a preconditioner, with the Chebyshev polynomial preconditioner at 16 steps and with the geometric
multigrid preconditioner; ONE configuration per invocation, so that a job runs each under a time limit of its own and chains
them:

    python scripts/mg_headline.py --case lap   --config none         # the base: first, the Chebyshev row reads its eigenvalues
    python scripts/mg_headline.py --case lap   --config chebyshev
    python scripts/mg_headline.py --case lap   --config multigrid
    python scripts/mg_headline.py --case lap3d --config none  ...

Every invocation adds (or replaces) its row in profiles/mg_headline.json (--out): the seconds of each of --repeats solves after
a 50-iteration warm-up solve of the same configuration, their median, outer iterations, matvecs, the preconditioner's counters
and the largest eigenvalue error against the analytic spectrum.  The multigrid row also times the V-cycle by itself: the
median of 20 applications to one vector, the bytes a cycle moves (every launch's streamed panels, counted by the rule in
vcycle_bytes below) and what fraction of the HBM peak (--peak, TB/s) that is.

Cases
  lap    the headline problem: 5-point Laplacian 3162 x 3163 (lap2d_10m), 10 smallest, GD+k, block 1, eps 1e-8 |A|, |A| = 8
  lap3d  BASELINE configs[1]: 7-point Laplacian 125 x 126 x 127, same settings, |A| = 12
  --small shrinks both (316 x 317; 40 x 41 x 42): a functional check.
The Chebyshev interval follows scripts/cheb_headline.py: lo = theta_k + (theta_k - theta_1)/k from the base solve's values."""
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


def mg_levels(lib, dims):
    n = np.zeros((24, 3), dtype=np.int32)
    w = np.zeros((24, 3))
    nl = C.c_int(0)
    assert lib.primme_amd_mg_plan((C.c_int * 3)(*dims), C.byref(nl), n.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p)) == 0
    return [tuple(int(v) for v in r) for r in n[:nl.value]]


def vcycle_bytes(levels, nu, ncs, es):
    """bytes one V(nu, nu) cycle streams for one vector: every panel a launch reads or writes once, neighbours from cache.
    A Chebyshev step from zero reads b and, from the second on, y_k (the third on: y_k-1) and writes one panel; the residual
    reads b, y and writes r; the restriction reads r and writes the coarse b; the interpolation reads the coarse y and reads and
    writes y; a step from y reads b, y_k (from the second on: y_k-1) and writes one panel."""
    def zero_start(m, steps):
        if steps == 1:
            return 2 * m
        return sum(min(k + 1, 4) * m for k in range(1, steps))

    total = 0
    for l, n in enumerate(levels):
        m = int(np.prod(n))
        if l == len(levels) - 1:
            total += zero_start(m, ncs)
            break
        mc = int(np.prod(levels[l + 1]))
        total += zero_start(m, nu) + 3 * m + (m + mc) + (mc + 2 * m)
        total += sum((3 if j == 1 else 4) * m for j in range(1, nu + 1))
    return total * es


def time_vcycle(s, n, reps=20):
    """median seconds of one application of the configured preconditioner to one vector (the operator's own stream, drained)"""
    import torch
    x = torch.randn(n, dtype=torch.float64, device="cuda")
    y = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    p = F.PrimmeParams()
    p.preconditioner = s.oph
    ld, bs, ierr = F.PRIMME_INT(n), C.c_int(1), C.c_int(0)
    ctx = dict(s.handles)["ctx"]

    def once():
        s.lib.primme_amd_multigrid_precond(C.c_void_p(x.data_ptr()), C.byref(ld), C.c_void_p(y.data_ptr()), C.byref(ld), C.byref(bs),
                                           C.byref(p), C.byref(ierr))
        assert ierr.value == 0 and s.lib.hipk_sync(ctx) == 0
    once()
    secs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        once()
        secs.append(time.perf_counter() - t0)
    return float(np.median(secs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("lap", "lap3d"), required=True)
    ap.add_argument("--config", choices=("none", "chebyshev", "multigrid"), required=True)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mg_headline.json"))
    ap.add_argument("--peak", type=float, default=8.0, help="HBM peak in TB/s the V-cycle's bandwidth is quoted against")
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    nev = 10
    if a.case == "lap":
        dims, aN = ((316, 317) if a.small else (3162, 3163)), 8.0
    else:
        dims, aN = ((40, 41, 42) if a.small else (125, 126, 127)), 12.0
    rp, ci, va, n = problems.laplacian_csr(dims)
    exact = problems.laplacian_eigenvalues(dims, nev)
    workload = f"{2 * len(dims) + 1}-point Laplacian {' x '.join(map(str, dims))}, {nev} smallest, GD+k, eps 1e-8 |A|"
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rows = doc.setdefault(a.case, dict(workload=workload, rows=[]))["rows"]
    s = Session(Operator(n, csr=(rp, ci, va)))
    kw = dict(numEvals=nev, target="smallest", method="GD_plusK", eps=1e-8, aNorm=aN, v0=problems.start_vector(n), return_evecs=False,
              maxOuterIterations=60000)
    if a.config == "none":
        label, precond = "none", None
    elif a.config == "chebyshev":
        base = [r for r in rows if r["label"] == "none"]
        if not base:
            raise SystemExit(f"{a.out} has no 'none' row for case {a.case}: run --config none first")
        th = np.sort(np.array(base[0]["evals"]))
        label, precond = "chebyshev steps=16", ("chebyshev", 16, float(th[-1] + (th[-1] - th[0]) / nev))
    else:
        label, precond = "multigrid V(2,2)", ("multigrid", dims, 2, 16)
    s.solve(precond=precond, **dict(kw, maxOuterIterations=50))      # warm-up, not timed
    secs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        r = s.solve(precond=precond, **kw)              # returns after the device has finished (the results are on the host)
        secs.append(time.perf_counter() - t0)
    row = dict(label=label, precond=[list(v) if isinstance(v, tuple) else v for v in precond] if precond else None, ret=r.ret,
               seconds=secs, seconds_median=float(np.median(secs)), outer_iterations=r.stats["numOuterIterations"],
               matvecs=r.stats["numMatvecs"], precond_stats=r.precond_stats,
               max_eval_error_vs_truth=float(np.max(np.abs(np.sort(r.evals) - exact))), evals=np.sort(r.evals).tolist())
    if a.config == "multigrid":
        levels = mg_levels(s.lib, (list(dims) + [1, 1])[:3])
        t = time_vcycle(s, n)
        nbytes = vcycle_bytes(levels, 2, 16, 8)
        row.update(levels=len(levels), vcycle_us=t * 1e6, vcycle_bytes=nbytes, vcycle_fine_grid_passes=nbytes / (8.0 * n),
                   vcycle_tb_per_s=nbytes / t / 1e12, hbm_peak_tb_per_s=a.peak, vcycle_fraction_of_hbm_peak=nbytes / t / 1e12 / a.peak,
                   launches_per_vcycle=r.precond_stats["launches"] / max(r.precond_stats["applies"], 1))
    s.close()
    rows[:] = [x for x in rows if x["label"] != label] + [row]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps({k: v for k, v in row.items() if k != "evals"}), flush=True)


if __name__ == "__main__":
    main()
