/* ex_eigs_dhip_cheb.c — the problem of ex_eigs_dhip.c (1-D Laplacian n = 100, 10 smallest eigenvalues, eps 1e-9) solved
 * with GD+k twice through the C ABI of libprimme_amd.so: without a preconditioner and with the Chebyshev polynomial
 * preconditioner primme_amd_chebyshev_precond (8 steps, the solver's shifts).  The interval to damp is [lo, hi]: lo = 0.11
 * lies in the gap above the ten wanted eigenvalues (the tenth is 0.0960, the eleventh 0.1158), hi is left to the
 * operator's Gershgorin bound (NAN).  Prints both outer-iteration counts.
 *
 *   make -C examples && examples/ex_eigs_dhip_cheb     (exit code 0 = both solves match 2 - 2cos(k pi/(n+1)) and the
 *                                                        preconditioned one took fewer outer iterations)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "primme_amd.h"
#include "primme_amd_kernels.h"
#include "primme_amd_comm.h"

static int solve(primme_amd_operator *op, hipk_ctx *ctx, int n, int nev, int cheb, long long *outer) {
   primme_params primme;
   primme_initialize(&primme);
   primme.n = n;
   primme.numEvals = nev;
   primme.eps = 1e-9;
   primme.target = primme_smallest;
   primme.matrix = op;
   primme.matrixMatvec = primme_amd_matvec;
   if (cheb) {
      if (primme_amd_operator_set_chebyshev(op, 8, 0.11, NAN, 0, 0.0)) return 1;
      primme.preconditioner = op;
      primme.applyPreconditioner = primme_amd_chebyshev_precond;
      primme.correctionParams.precondition = 1;
   }
   primme_set_method(PRIMME_GD_plusK, &primme);

   double evals[10], rnorms[10], *evecs_dev;
   if (hipk_malloc(ctx, sizeof(double) * n * nev, (void **)&evecs_dev)) return 2;
   primme_amd_chebyshev_stats(NULL, NULL, NULL);
   const int ret = hip_dprimme(evals, evecs_dev, rnorms, &primme);
   long applies = 0, products = 0, fused = 0;
   primme_amd_chebyshev_stats(&applies, &products, &fused);
   int bad = (ret != 0 || primme.initSize != nev);
   printf("%s: hip_dprimme returned %d, %d pairs, %lld outer iterations, %lld matvecs, %ld vectors preconditioned with %ld operator products (%ld fused)\n",
         cheb ? "chebyshev" : "plain", ret, primme.initSize, (long long)primme.stats.numOuterIterations, (long long)primme.stats.numMatvecs,
         applies, products, fused);
   for (int k = 0; k < primme.initSize; k++)
      if (fabs(evals[k] - (2.0 - 2.0 * cos((k + 1) * M_PI / (n + 1)))) > 1e-10 * 4.0) bad = 1;
   *outer = (long long)primme.stats.numOuterIterations;
   hipk_free(ctx, evecs_dev);
   primme_free(&primme);
   return bad;
}

int main(void) {
   const int n = 100, nev = 10;
   int32_t *rp = malloc(sizeof(int32_t) * (n + 1)), *ci = malloc(sizeof(int32_t) * 3 * n);
   double *va = malloc(sizeof(double) * 3 * n);
   int nnz = 0;
   for (int i = 0; i < n; i++) {
      rp[i] = nnz;
      if (i > 0) { ci[nnz] = i - 1; va[nnz++] = -1.0; }
      ci[nnz] = i; va[nnz++] = 2.0;
      if (i < n - 1) { ci[nnz] = i + 1; va[nnz++] = -1.0; }
   }
   rp[n] = nnz;

   hipk_ctx *ctx;
   hipk_csr *A;
   primme_amd_operator *op;
   if (hipk_ctx_create(&ctx, NULL)) { fprintf(stderr, "no HIP device\n"); return 2; }
   if (hipk_csr_create(ctx, HIPK_F64, n, n, 0, rp, ci, va, &A)) return 2;
   if (primme_amd_operator_create(&op, A, NULL)) return 2;

   long long plain = 0, pre = 0;
   int bad = solve(op, ctx, n, nev, 0, &plain);
   bad |= solve(op, ctx, n, nev, 1, &pre);
   printf("outer iterations without preconditioner: %lld\nouter iterations with the Chebyshev preconditioner: %lld\n", plain, pre);
   if (!(pre < plain)) bad = 1;

   primme_amd_operator_destroy(op);
   hipk_csr_destroy(A);
   hipk_ctx_destroy(ctx);
   free(rp); free(ci); free(va);
   return bad;
}
