/* ex_eigs_dhip_amg_reuse.c — one algebraic multigrid hierarchy, two solves.  A symmetric positive definite Matrix-Market matrix
 * (the tests pass tests/golden/reference_driver/LUNDA.mtx), optionally tiled block-diagonally ntiles times (tile t scaled by
 * 1 + t / 4) so that the hierarchy has more than one level.  The hierarchy of smoothed aggregation is built ONCE, its
 * row-parallel stages on the device (primme_amd_amg_hierarchy_create, setup 1), and attached to two GD+k solves with different
 * numEvals (4, then 2) and different smoothers (V(2,2), then V(1,1)): the set-up seconds are printed once, the outer iterations
 * of both solves after them.
 *
 *   make -C examples && examples/ex_eigs_dhip_amg_reuse matrix.mtx [ntiles]     (exit code 0 = both solves converged)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "primme_amd.h"
#include "primme_amd_kernels.h"
#include "primme_amd_comm.h"
#include "primme_amd_io.h"

#define MAXEV 4

static int solve(primme_amd_operator *op, struct primme_amd_amg_hierarchy *h, hipk_ctx *ctx, int n, double aNorm, int nev, int steps,
      double *evals, long long *outer) {
   primme_params primme;
   primme_initialize(&primme);
   primme.n = n;
   primme.numEvals = nev;
   primme.eps = 1e-10;
   primme.aNorm = aNorm;
   primme.target = primme_smallest;
   primme.matrix = op;
   primme.matrixMatvec = primme_amd_matvec;
   primme.preconditioner = op;
   primme.correctionParams.precondition = 1;
   if (primme_amd_operator_set_amg_hierarchy(op, h, steps, 16, 1.0)) return 1;      /* the smoother belongs to the attachment */
   primme.applyPreconditioner = primme_amd_amg_precond;
   primme_set_method(PRIMME_GD_plusK, &primme);

   double rnorms[MAXEV], *evecs_dev;
   if (hipk_malloc(ctx, sizeof(double) * n * nev, (void **)&evecs_dev)) return 2;
   primme_amd_amg_stats(NULL, NULL, NULL);
   const int ret = hip_dprimme(evals, evecs_dev, rnorms, &primme);
   long applies = 0, launches = 0, levels = 0;
   primme_amd_amg_stats(&applies, &launches, &levels);
   int bad = (ret != 0 || primme.initSize != nev);
   printf("%d pairs, V(%d,%d): hip_dprimme returned %d, %d pairs, %lld outer iterations, %ld vectors preconditioned on %ld levels\n", nev, steps, steps,
         ret, primme.initSize, (long long)primme.stats.numOuterIterations, applies, levels);
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
   const int ntiles = argc > 2 ? atoi(argv[2]) : 1;
   if (argc < 2 || argc > 3 || ntiles < 1) { fprintf(stderr, "usage: %s matrix.mtx [ntiles]\n", argv[0]); return 2; }
   int64_t m, n, nnz;
   int32_t *rp, *ci;
   double *va;
   int is_complex = 0;
   if (primme_amd_mm_read(argv[1], &m, &n, &nnz, &rp, &ci, &va, &is_complex) || is_complex || m != n) {
      fprintf(stderr, "%s: not a real square Matrix-Market matrix\n", argv[1]);
      return 2;
   }
   if (ntiles > 1) {
      int32_t *rp2, *ci2;
      double *va2;
      if (primme_amd_csr_tile_block_diagonal(n, rp, ci, va, ntiles, 0, 1.0, 0.25, &rp2, &ci2, &va2)) return 2;
      primme_amd_host_free(rp); primme_amd_host_free(ci); primme_amd_host_free(va);
      rp = rp2; ci = ci2; va = va2;
      n *= ntiles;
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
   struct primme_amd_amg_hierarchy *h;
   if (hipk_ctx_create(&ctx, NULL)) { fprintf(stderr, "no HIP device\n"); return 2; }
   if (hipk_csr_create(ctx, HIPK_F64, n, n, 0, rp, ci, va, &A)) return 2;
   if (primme_amd_operator_create(&op, A, NULL)) return 2;
   if (primme_amd_amg_hierarchy_create(op, rp, ci, va, 1, 0.08, 4.0 / 3.0, 0.0, 1, &h)) { fprintf(stderr, "the hierarchy could not be built\n"); return 2; }

   int nlevels = 0, fallback = 0;
   int64_t rows[PRIMME_AMD_AMG_MAXLEVELS];
   double setup = 0.0, device = 0.0;
   primme_amd_amg_hierarchy_info(h, &nlevels, rows, NULL, NULL, &setup, &device, NULL);
   primme_amd_amg_hierarchy_stages(h, &fallback, NULL);
   printf("hierarchy set-up: %.6f seconds (%.6f in the device stages), %d levels, rows", setup, device, nlevels);
   for (int l = 0; l < nlevels; l++) printf(" %lld", (long long)rows[l]);
   printf(", %d levels built on the host\n", fallback);

   long long first = 0, second = 0;
   long attached = 0;
   double e1[MAXEV], e2[MAXEV];
   int bad = solve(op, h, ctx, (int)n, aNorm, 4, 2, e1, &first);
   bad |= solve(op, h, ctx, (int)n, aNorm, 2, 1, e2, &second);
   primme_amd_amg_hierarchy_info(h, NULL, NULL, NULL, NULL, NULL, NULL, &attached);
   printf("outer iterations of the first solve: %lld\nouter iterations of the second solve: %lld\nthe hierarchy was attached %ld times\n", first, second,
         attached);
   for (int k = 0; k < 2; k++)
      if (!(fabs(e1[k] - e2[k]) <= 2e-10 * aNorm)) bad = 1;      /* each within its residual bound eps |A| of an eigenvalue */

   primme_amd_amg_hierarchy_destroy(h);         /* the operator still holds it; it goes with the operator */
   primme_amd_operator_destroy(op);
   hipk_csr_destroy(A);
   hipk_ctx_destroy(ctx);
   primme_amd_host_free(rp); primme_amd_host_free(ci); primme_amd_host_free(va);
   return bad;
}
