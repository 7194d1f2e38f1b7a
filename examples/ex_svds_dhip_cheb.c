/* ex_svds_dhip_cheb.c — the three smallest singular values of the (n+1) x n difference matrix D (D[i,i] = 1, D[i+1,i] = -1;
 * sigma_k = 2 sin(k pi / (2 (n+1)))) through the C ABI, without a preconditioner and with the Chebyshev polynomial
 * preconditioner of primme_amd_svds.h.  Every row and column of D has the same sum of squares (but the two ends), so the
 * Jacobi preconditioner does nothing here; the polynomial one trades products inside K^-1 for outer iterations.
 *   make -C examples && examples/ex_svds_dhip_cheb */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "primme_amd_svds.h"
#include "primme_amd_kernels.h"

#define K 3

static int solve(primme_amd_svds_operator *op, hipk_ctx *ctx, int m, int n, int cheb, double *svals, long long *outer) {
   primme_svds_params ps;
   primme_svds_initialize(&ps);
   ps.m = m; ps.n = n; ps.numSvals = K; ps.eps = 1e-8; ps.target = primme_svds_smallest; ps.printLevel = 0;
   ps.matrix = op;
   ps.matrixMatvec = primme_amd_svds_matvec;
   if (cheb) {
      /* damp the singular values in [0.011, norm bound] (sigma_3 = 0.0094 < 0.011 < sigma_4 = 0.0126), target 0 */
      if (primme_amd_svds_operator_set_chebyshev(op, 16, 0.011, NAN, 0.0)) return -1;
      ps.preconditioner = op;
      ps.applyPreconditioner = primme_amd_svds_chebyshev_precond;
   }
   primme_svds_set_method(primme_svds_normalequations, PRIMME_GD_plusK, PRIMME_DEFAULT_METHOD, &ps);
   double rnorms[K], *svecs_dev;
   if (hipk_malloc(ctx, sizeof(double) * (size_t)(m + n) * K, (void **)&svecs_dev)) return -1;
   primme_amd_chebyshev_stats(NULL, NULL, NULL);
   const int ret = hip_dprimme_svds(svals, svecs_dev, rnorms, &ps);
   hipk_free(ctx, svecs_dev);
   *outer = (long long)ps.stats.numOuterIterations;
   return (ret != 0 || ps.initSize != K) ? -1 : 0;
}

int main(void) {
   const int n = 1000, m = n + 1;
   int32_t *rp = malloc(sizeof(int32_t) * (m + 1)), *ci = malloc(sizeof(int32_t) * 2 * n);
   double *va = malloc(sizeof(double) * 2 * n);
   int nnz = 0;
   for (int i = 0; i < m; i++) {
      rp[i] = nnz;
      if (i > 0) { ci[nnz] = i - 1; va[nnz++] = -1.0; }
      if (i < n) { ci[nnz] = i; va[nnz++] = 1.0; }
   }
   rp[m] = nnz;

   hipk_ctx *ctx;
   primme_amd_svds_operator *op;
   if (hipk_ctx_create(&ctx, NULL)) { fprintf(stderr, "no HIP device\n"); return 2; }
   if (primme_amd_svds_operator_create(&op, ctx, HIPK_F64, m, n, rp, ci, va)) return 2;
   double bound = 0.0;
   if (primme_amd_svds_operator_norm_bound(op, &bound)) return 2;
   printf("norm bound sqrt(|D|_1 |D|_inf) = %g\n", bound);

   double s0[K], s1[K];
   long long it0 = 0, it1 = 0;
   long applies = 0, products = 0, fused = 0;
   int bad = solve(op, ctx, m, n, 0, s0, &it0) != 0;
   printf("outer iterations without preconditioner: %lld\n", it0);
   bad |= solve(op, ctx, m, n, 1, s1, &it1) != 0;
   primme_amd_chebyshev_stats(&applies, &products, &fused);
   printf("outer iterations with the Chebyshev preconditioner: %lld (%ld vectors preconditioned, %ld products inside)\n", it1, applies, products);
   for (int i = 0; i < K; i++) {
      const double exact = 2.0 * sin((i + 1) * acos(-1.0) / (2.0 * (n + 1)));
      printf("Sval[%d] = %-22.15E  %-22.15E  exact %-22.15E\n", i + 1, s0[i], s1[i], exact);
      if (fabs(s0[i] - exact) > 1e-7 * bound || fabs(s1[i] - exact) > 1e-7 * bound) bad = 1;
   }
   if (bound != 2.0 || products != 30 * applies) bad = 1;
   primme_amd_svds_operator_destroy(op);
   hipk_ctx_destroy(ctx);
   free(rp); free(ci); free(va);
   return bad;
}
