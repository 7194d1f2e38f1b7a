"""Generates tests/golden/reference_cheb.json: the REAL reference (oracle/_ref/libprimme_ref.so) on the cases of
tests/cheb_cases.py with the numpy restatement of the Chebyshev polynomial preconditioner as its applyPreconditioner.
Run in the build container only:  python tests/golden/make_cheb_golden.py"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cheb_cases as CC  # noqa: E402


def main():
    out = {}
    for name in sorted(CC.CASES):
        counter = [0]
        r = CC.run_case(name, "reference", counter)
        _, _, spec, _, anorm = CC.case_setup(name)
        out[name] = dict(ret=r.ret, initSize=r.initSize, evals=np.asarray(r.evals, dtype=np.float64).tolist(),
                         resNorms=np.asarray(r.resNorms, dtype=np.float64).tolist(), aNorm=anorm, cheb=spec, precond_applies=counter[0],
                         stats={k: r.stats[k] for k in ("numOuterIterations", "numMatvecs", "numRestarts", "numPreconds")})
        print(name, r.ret, r.initSize, out[name]["stats"], counter[0], r.evals)
    json.dump(out, open(CC.GOLDEN, "w"), indent=1)


if __name__ == "__main__":
    main()
