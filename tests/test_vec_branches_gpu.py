"""Every launch shape of csrc/hipk_vec.hip at small sizes (-m gpu): the cases of tests/vec_branch_cases.py on the device against
the longdouble references written from the header, with the derived bounds, the guard / padding comparison of every operand and
the bit-for-bit identities the header promises (fused pass against the separate calls, device recurrences against host
coefficients, second run against first).  One test per (entry point, type); the grid-cap case of each is a test of its own.  The
same cases run on the plain-C oracle in tests/test_vec_branches_host.py, which also asserts what the tables cover.

Largest error / bound on an MI355X and on the oracle when these files were written (entry point, type, cases: device / oracle;
the grid-cap case counted in): axpy f32 17: 0.12 / 0.12, f64 17: 0.12 / 0.23; axpy_dot (Z) f32 16: 0.12 / 0.12, f64 16: 0.12 / 0.24;
axpy_dot (Z == NULL) f32 16: 0.12 / 0.12, f64 16: 0.12 / 0.29; axpy_proj_dot f32 16: 0.083 / 0.083, f64 16: 0.22 / 0.28;
axpy_proj_dot_jacobi f32 21: 0.083 / 0.083, f64 21: 0.19 / 0.28; axpy_proj_dot_jacobi_dev f32 17: 0.083 / 0.083, f64 17: 0.17 / 0.28;
gather 17 and pair_rotate 16 per type: exact; jacobi f32, f64, c32, c64 18 each: 0.12 / 0.12; col_norms2 f32 16: 0.012 / 0.038,
f64 16: 0.12 / 0.12; pair_dots f32 16: 0.0044 / 0.015, f64 16: 0.052 / 0.052; qmr_update f32 16: 0.1 / 0.1, f64 16: 0.24 / 0.24;
qmr_update_dir f32 21: 0.1 / 0.1, f64 21: 0.24 / 0.24; qmr_update_dir_dev f32 17: 0.1 / 0.1, f64 17: 0.23 / 0.23;
qmr_update_jacobi f32 21: 0.12 / 0.12, f64 21: 0.24 / 0.24; residual_cols f32 17: 0.12 / 0.12, f64 17: 0.12 / 0.24;
scale f32, f64 17: 0.17 / 0.17; scale_rsqrt f32 16: 0.1 / 0.1, f64 16: 0.23 / 0.23; triple_dots f32 16: 0.0064 / 0.019,
f64 16: 0.12 / 0.12; xpay f32 17: 0.12 / 0.12, f64 17: 0.12 / 0.23.  Per layout flavour the ratios differ in the third digit
(the test prints them).  Columns that leave the block: 25 cases per type, return codes 33 per real and 13 per complex type: bits
only.  The reductions for which the header promises no bit equality with the unfused call (out[c] of qmr_update_jacobi,
axpy_proj_dot_jacobi, qmr_update_dir) agreed bit-wise in every case on both sides."""
import pytest

from kernel_harness import Dev
import vec_branch_cases as V

pytestmark = pytest.mark.gpu

GROUPS = V.groups()


@pytest.mark.parametrize("gid,cases", GROUPS, ids=[g for g, _ in GROUPS])
def test_device_against_longdouble_reference(built, gid, cases):
    rep = V.run_cases(Dev, cases)
    print(f"{gid}: {rep.summary()}")
    assert not rep.fails, f"{gid}: {rep.summary()}\n" + "\n".join(rep.fails[:20])
