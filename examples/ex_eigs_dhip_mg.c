/* ex_eigs_dhip_mg.c — the 5-point Laplacian on a 63 x 65 grid (n = 4095, matrix-free stencil operator), 6 smallest
 * eigenvalues, eps 1e-10, solved with GD+k twice through the C ABI of libprimme_amd.so: without a preconditioner and with
 * the geometric multigrid preconditioner primme_amd_multigrid_precond (one V(2,2) cycle per vector, 16 Chebyshev steps on the
 * coarsest grid, scale 1, shift 0: K^-1 approximates the inverse of the Laplacian itself).  Prints both outer-iteration
 * counts.
 *
 *   make -C examples && examples/ex_eigs_dhip_mg     (exit code 0 = both solves match the analytic eigenvalues and the
 *                                                      preconditioned one took fewer outer iterations)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "primme_amd.h"
#include "primme_amd_kernels.h"
#include "primme_amd_comm.h"

#define NX 63
#define NY 65
#define NEV 6

static int cmp(const void *a, const void *b) { return *(const double *)a < *(const double *)b ? -1 : *(const double *)a > *(const double *)b; }

static int solve(primme_amd_operator *op, hipk_ctx *ctx, const double *exact, int mg, long long *outer) {
   const int n = NX * NY;
   primme_params primme;
   primme_initialize(&primme);
   primme.n = n;
   primme.numEvals = NEV;
   primme.eps = 1e-10;
   primme.aNorm = 8.0;
   primme.target = primme_smallest;
   primme.matrix = op;
   primme.matrixMatvec = primme_amd_matvec;
   if (mg) {
      if (primme_amd_operator_set_multigrid(op, NX, NY, 1, 2, 16, 1.0, 0.0)) return 1;
      primme.preconditioner = op;
      primme.applyPreconditioner = primme_amd_multigrid_precond;
      primme.correctionParams.precondition = 1;
   }
   primme_set_method(PRIMME_GD_plusK, &primme);

   double evals[NEV], rnorms[NEV], *evecs_dev;
   if (hipk_malloc(ctx, sizeof(double) * n * NEV, (void **)&evecs_dev)) return 2;
   primme_amd_multigrid_stats(NULL, NULL);
   const int ret = hip_dprimme(evals, evecs_dev, rnorms, &primme);
   long applies = 0, launches = 0;
   primme_amd_multigrid_stats(&applies, &launches);
   int bad = (ret != 0 || primme.initSize != NEV);
   printf("%s: hip_dprimme returned %d, %d pairs, %lld outer iterations, %lld matvecs, %ld vectors preconditioned in %ld kernel launches\n",
         mg ? "multigrid" : "plain", ret, primme.initSize, (long long)primme.stats.numOuterIterations, (long long)primme.stats.numMatvecs,
         applies, launches);
   for (int k = 0; k < primme.initSize; k++)
      if (fabs(evals[k] - exact[k]) > 1e-9 * 8.0) bad = 1;
   *outer = (long long)primme.stats.numOuterIterations;
   hipk_free(ctx, evecs_dev);
   primme_free(&primme);
   return bad;
}

int main(void) {
   /* the analytic spectrum: 4 - 2cos(i pi/(NX+1)) - 2cos(j pi/(NY+1)); the smallest lie among the first few i, j */
   double lam[64];
   for (int i = 1; i <= 8; i++)
      for (int j = 1; j <= 8; j++) lam[(i - 1) * 8 + j - 1] = 4.0 - 2.0 * cos(i * M_PI / (NX + 1)) - 2.0 * cos(j * M_PI / (NY + 1));
   qsort(lam, 64, sizeof(double), cmp);

   hipk_ctx *ctx;
   hipk_csr *A;
   primme_amd_operator *op;
   if (hipk_ctx_create(&ctx, NULL)) { fprintf(stderr, "no HIP device\n"); return 2; }
   if (hipk_stencil_create(ctx, HIPK_F64, NX, NY, 1, 0, NX * NY, &A)) return 2;
   if (primme_amd_operator_create(&op, A, NULL)) return 2;

   long long plain = 0, pre = 0;
   int bad = solve(op, ctx, lam, 0, &plain);
   bad |= solve(op, ctx, lam, 1, &pre);
   printf("outer iterations without preconditioner: %lld\nouter iterations with the multigrid preconditioner: %lld\n", plain, pre);
   if (!(pre < plain)) bad = 1;

   primme_amd_operator_destroy(op);
   hipk_csr_destroy(A);
   hipk_ctx_destroy(ctx);
   return bad;
}
