"""BASELINE configs[4] (8e6 x 2e6, 5 entries per row, 10 largest singular triplets, normal equations, GD+k) without a
preconditioner and with the Chebyshev polynomial preconditioner of include/primme_amd_svds.h; ONE configuration per invocation,
so that a job runs each under a time limit of its own and chains them:

    python scripts/svds_cheb_config4.py --config none          # the base: always first, the others read its row
    python scripts/svds_cheb_config4.py --config 4             # steps = 4, then 8, 16

Every invocation adds (or replaces) its row in profiles/svds_cheb_config4.json (--out): the seconds of each of --repeats solves
(default 2) after a warm-up solve of the same configuration, their median, outer iterations, matvecs, the operator products
inside the preconditioner and the largest singular value error against the base solve.

Rule for the interval (no knowledge of the spectrum beyond the base solve): with s_1 >= ... >= s_k the wanted singular values the
base solve returned and g = (s_1 - s_k)/k their mean spacing: slo = 0, shi = s_k - g, sshift = the norm bound sqrt(|A|_1 |A|_inf)
(left to the library).  --small shrinks the matrix to 80 000 x 20 000: a functional check."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from primme_amd import problems  # noqa: E402
from primme_amd.svds_api import SvdsSession  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", required=True, help="none, or the number of steps")
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svds_cheb_config4.json"))
    ap.add_argument("--small", action="store_true")
    a = ap.parse_args()
    m, n, k = (80_000, 20_000, 10) if a.small else (8_000_000, 2_000_000, 10)
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}
    doc.setdefault("workload", f"configs[4]: A {m} x {n} CSR, 5 entries per row; {k} largest singular triplets, normal equations, GD+k, eps 1e-8 |A|")
    rows = doc.setdefault("rows", [])
    base = [r for r in rows if r["label"] == "none"]
    if a.config == "none":
        label, precond = "none", None
    else:
        if not base:
            raise SystemExit(f"{a.out} has no 'none' row: run --config none first")
        s = np.sort(np.array(base[0]["svals"]))[::-1]
        g = (s[0] - s[-1]) / k
        precond = ("chebyshev", int(a.config), 0.0, float(s[-1] - g))
        label = f"chebyshev steps={a.config}"
    sess = SvdsSession(m, n, problems.svds_synthetic_csr(m, n))
    kw = dict(numSvals=k, eps=1e-8, methodStage1="GD_plusK", precond=precond)
    sess.solve(**kw)                                      # warm-up, not timed
    secs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        r = sess.solve(**kw)                              # returns after the device has finished (the results are on the host)
        secs.append(time.perf_counter() - t0)
    sess.close()
    st = r.precond_stats or dict(applies=0, operator_products=0, fused_steps=0)
    sv = np.sort(np.asarray(r.svals, dtype=np.float64))[::-1]
    err = float(np.max(np.abs(sv - np.sort(np.array(base[0]["svals"]))[::-1]))) if base and a.config != "none" else 0.0
    row = dict(label=label, precond=list(precond) if precond else None, ret=r.ret, triplets=r.initSize, seconds=secs,
               seconds_median=float(np.median(secs)), outer_iterations=r.stats["numOuterIterations"], matvecs=r.stats["numMatvecs"],
               preconds=r.stats["numPreconds"], operator_products_in_precond=st["operator_products"], fused_steps=st["fused_steps"],
               max_sval_error_vs_base=err, aNorm=float(r.params["aNorm"]), max_res_norm=float(np.max(r.resNorms)), svals=sv.tolist())
    rows[:] = [x for x in rows if x["label"] != label] + [row]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(doc, open(a.out, "w"), indent=1)
    print(json.dumps({kk: v for kk, v in row.items() if kk != "svals"}), flush=True)


if __name__ == "__main__":
    main()
