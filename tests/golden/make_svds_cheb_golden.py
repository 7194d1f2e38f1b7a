"""Generates tests/golden/reference_svds_cheb.json: the REAL reference (oracle/_ref/libprimme_ref.so, dprimme_svds /
sprimme_svds / zprimme_svds) on the cases of tests/svds_cheb_cases.py with the numpy restatement of the Chebyshev
polynomial preconditioner as its applyPreconditioner, and the unpreconditioned solve of every case.
Run in the build container only:  python tests/golden/make_svds_cheb_golden.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svds_cheb_cases as SC  # noqa: E402

KEYS = ("numOuterIterations", "numMatvecs", "numRestarts", "numPreconds")


def record(r):
    return dict(ret=r.ret, initSize=r.initSize, svals=np.asarray(r.svals, dtype=np.float64).tolist(),
                resNorms=np.asarray(r.resNorms, dtype=np.float64).tolist(), aNorm=float(r.params["aNorm"]),
                stats={k: r.stats[k] for k in KEYS})


def main():
    out = {}
    for name in sorted(SC.CASES):
        counter = [0]
        r = SC.run_case(name, "reference", counter)
        plain = SC.run_case(name, "reference", plain=True)
        hc = SC.run_case(name, "hostcheck")
        _, _, _, _, spec, _, s0, _ = SC.case_setup(name)
        out[name] = dict(record(r), norm2=s0, cheb=spec, precond_applies=counter[0], plain=record(plain),
                         hostcheck_outer_iterations=hc.stats["numOuterIterations"])
        print(name, r.ret, r.initSize, out[name]["stats"], counter[0], "plain", out[name]["plain"]["stats"], r.svals)
    json.dump(out, open(SC.GOLDEN, "w"), indent=1)


if __name__ == "__main__":
    main()
