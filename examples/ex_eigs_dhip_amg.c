/* ex_eigs_dhip_amg.c — a symmetric positive definite Matrix-Market matrix (the tests pass the structural matrix
 * tests/golden/reference_driver/LUNDA.mtx), 4 smallest eigenvalues, eps 1e-10, solved with GD+k twice through the C ABI of
 * libprimme_amd.so: with the Jacobi preconditioner and with the aggregation algebraic multigrid preconditioner
 * primme_amd_amg_precond (one V(2,2) cycle per vector on a hierarchy that the library aggregates from the CSR arrays; theta
 * 0.08, over 1, shift 0).  Prints both outer-iteration counts.  With --smoothed after the matrix the second solve uses the
 * hierarchy of smoothed aggregation instead (primme_amd_operator_set_amg_smoothed, omega 4/3).
 *
 *   make -C examples && examples/ex_eigs_dhip_amg matrix.mtx [--smoothed]     (exit code 0 = both solves converged to the same
 *   eigenvalues)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "primme_amd.h"
#include "primme_amd_kernels.h"
#include "primme_amd_comm.h"
#include "primme_amd_io.h"

#define NEV 4

static int solve(primme_amd_operator *op, hipk_ctx *ctx, int n, double aNorm, const int32_t *rp, const int32_t *ci, const double *va,
      int amg, double *evals, long long *outer) {
   primme_params primme;
   primme_initialize(&primme);
   primme.n = n;
   primme.numEvals = NEV;
   primme.eps = 1e-10;
   primme.aNorm = aNorm;
   primme.target = primme_smallest;
   primme.matrix = op;
   primme.matrixMatvec = primme_amd_matvec;
   primme.preconditioner = op;
   primme.correctionParams.precondition = 1;
   if (amg) {
      if (amg == 2 ? primme_amd_operator_set_amg_smoothed(op, rp, ci, va, 2, 16, 0.08, 4.0 / 3.0, 0.0)
                   : primme_amd_operator_set_amg(op, rp, ci, va, 2, 16, 0.08, 1.0, 0.0)) return 1;
      primme.applyPreconditioner = primme_amd_amg_precond;
   } else {
      primme_amd_operator_set_jacobi(op, 0, 0.0);              /* K = diag(A) - the solver's shift of each vector */
      primme.applyPreconditioner = primme_amd_jacobi_precond;
   }
   primme_set_method(PRIMME_GD_plusK, &primme);

   double rnorms[NEV], *evecs_dev;
   if (hipk_malloc(ctx, sizeof(double) * n * NEV, (void **)&evecs_dev)) return 2;
   primme_amd_amg_stats(NULL, NULL, NULL);
   const int ret = hip_dprimme(evals, evecs_dev, rnorms, &primme);
   long applies = 0, launches = 0, levels = 0;
   primme_amd_amg_stats(&applies, &launches, &levels);
   int bad = (ret != 0 || primme.initSize != NEV);
   printf("%s: hip_dprimme returned %d, %d pairs, %lld outer iterations, %lld matvecs", amg == 2 ? "amg (smoothed)" : amg ? "amg" : "jacobi", ret, primme.initSize,
         (long long)primme.stats.numOuterIterations, (long long)primme.stats.numMatvecs);
   if (amg) printf(", %ld vectors preconditioned in %ld launches on %ld levels", applies, launches, levels);
   printf("\n");
   for (int k = 0; k < primme.initSize; k++) {
      printf("   lambda[%d] = %.12e  residual %.3e\n", k, evals[k], rnorms[k]);
      if (!(rnorms[k] <= 1e-10 * aNorm)) bad = 1;
   }
   *outer = (long long)primme.stats.numOuterIterations;
   hipk_free(ctx, evecs_dev);
   primme_free(&primme);
   return bad;
}

int main(int argc, char **argv) {
   if (argc < 2 || (argc > 2 && strcmp(argv[2], "--smoothed"))) { fprintf(stderr, "usage: %s matrix.mtx [--smoothed]\n", argv[0]); return 2; }
   const int smoothed = argc > 2;
   int64_t m, n, nnz;
   int32_t *rp, *ci;
   double *va;
   int is_complex = 0;
   if (primme_amd_mm_read(argv[1], &m, &n, &nnz, &rp, &ci, &va, &is_complex) || is_complex || m != n) {
      fprintf(stderr, "%s: not a real square Matrix-Market matrix\n", argv[1]);
      return 2;
   }
   double aNorm = 0.0;                          /* the largest absolute row sum bounds |A| */
   for (int64_t i = 0; i < n; i++) {
      double s = 0.0;
      for (int32_t q = rp[i]; q < rp[i + 1]; q++) s += fabs(va[q]);
      if (s > aNorm) aNorm = s;
   }

   hipk_ctx *ctx;
   hipk_csr *A;
   primme_amd_operator *op;
   if (hipk_ctx_create(&ctx, NULL)) { fprintf(stderr, "no HIP device\n"); return 2; }
   if (hipk_csr_create(ctx, HIPK_F64, n, n, 0, rp, ci, va, &A)) return 2;
   if (primme_amd_operator_create(&op, A, NULL)) return 2;

   long long jac = 0, amg = 0;
   double ej[NEV], ea[NEV];
   int bad = solve(op, ctx, (int)n, aNorm, rp, ci, va, 0, ej, &jac);
   bad |= solve(op, ctx, (int)n, aNorm, rp, ci, va, smoothed ? 2 : 1, ea, &amg);
   printf("outer iterations with the Jacobi preconditioner: %lld\nouter iterations with the algebraic multigrid preconditioner: %lld\n", jac, amg);
   for (int k = 0; k < NEV; k++)
      if (!(fabs(ej[k] - ea[k]) <= 2e-10 * aNorm)) bad = 1;      /* each within its residual bound eps |A| of an eigenvalue */

   primme_amd_operator_destroy(op);
   hipk_csr_destroy(A);
   hipk_ctx_destroy(ctx);
   primme_amd_host_free(rp); primme_amd_host_free(ci); primme_amd_host_free(va);
   return bad;
}
