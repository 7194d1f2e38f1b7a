/* ex_eigs_dhip_potential.c — a 2-D harmonic oscillator, H = -1/2 Laplacian + 1/2 omega^2 r^2, on a 48 x 48 grid with
 * Dirichlet walls, through the C ABI of libprimme_amd.so: the six smallest eigenvalues with GD+k and the Jacobi (Davidson)
 * preconditioner.  Multiplied by 2 h^2 the matrix is the 5-point Laplacian (4, -1) plus the diagonal w^2 rho^2, w = h^2 omega,
 * rho the distance from the centre in grid units; its eigenvalues approach 2 w (i + j + 1), i, j = 0, 1, ...
 *
 * The diagonal differs from row to row, so no two rows repeat; created with hipk_csr_create_opts(HIPK_CSR_DIAG_PATTERNS) the
 * matrix still takes the row-pattern form of the one-column products (one byte per row + the streamed diagonal): the rows
 * repeat but for their diagonal entry.  hipk_csr_pattern_diag reports it.
 *
 *   make -C examples && examples/ex_eigs_dhip_potential   (exit code 0 = six converged pairs in the diagonal-split form)
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "primme_amd.h"
#include "primme_amd_kernels.h"
#include "primme_amd_comm.h"

int main(void) {
   const int nx = 48, ny = 48, n = nx * ny, nev = 6;
   const double w = 0.05, cx = 0.5 * (nx - 1), cy = 0.5 * (ny - 1);
   int32_t *rp = malloc(sizeof(int32_t) * (n + 1)), *ci = malloc(sizeof(int32_t) * 5 * n);
   double *va = malloc(sizeof(double) * 5 * n);
   int nnz = 0;
   for (int iy = 0; iy < ny; iy++)
      for (int ix = 0; ix < nx; ix++) {
         const int i = iy * nx + ix;
         const double dx = ix - cx, dy = iy - cy;
         rp[i] = nnz;
         if (iy > 0) { ci[nnz] = i - nx; va[nnz++] = -1.0; }
         if (ix > 0) { ci[nnz] = i - 1; va[nnz++] = -1.0; }
         ci[nnz] = i; va[nnz++] = 4.0 + w * w * (dx * dx + dy * dy);
         if (ix < nx - 1) { ci[nnz] = i + 1; va[nnz++] = -1.0; }
         if (iy < ny - 1) { ci[nnz] = i + nx; va[nnz++] = -1.0; }
      }
   rp[n] = nnz;

   hipk_ctx *ctx;
   hipk_csr *A;
   primme_amd_operator *op;
   if (hipk_ctx_create(&ctx, NULL)) { fprintf(stderr, "no HIP device\n"); return 2; }
   if (hipk_csr_create_opts(ctx, HIPK_F64, n, n, 0, rp, ci, va, HIPK_CSR_DIAG_PATTERNS, &A)) return 2;
   if (primme_amd_operator_create(&op, A, NULL)) return 2;
   printf("one-column product: format %d, %d row patterns, diagonal streamed: %d, %.0f bytes per product\n", hipk_csr_format(A),
         hipk_csr_npatterns(A), hipk_csr_pattern_diag(A), hipk_csr_product_bytes(A, 0));

   primme_params primme;
   primme_initialize(&primme);
   primme.n = n;
   primme.numEvals = nev;
   primme.eps = 1e-9;
   primme.target = primme_smallest;
   primme.matrix = op;
   primme.matrixMatvec = primme_amd_matvec;
   primme_amd_operator_set_jacobi(op, 0, 0.0);              /* K = diag(A) - the solver's shift of each vector */
   primme.preconditioner = op;
   primme.applyPreconditioner = primme_amd_jacobi_precond;
   primme.correctionParams.precondition = 1;
   primme_set_method(PRIMME_GD_plusK, &primme);

   double evals[6], rnorms[6], *evecs_dev;
   if (hipk_malloc(ctx, sizeof(double) * n * nev, (void **)&evecs_dev)) return 2;
   const int ret = hip_dprimme(evals, evecs_dev, rnorms, &primme);
   int bad = (ret != 0 || primme.initSize != nev || hipk_csr_pattern_diag(A) != 1);
   printf("hip_dprimme returned %d, %d pairs, %lld outer iterations, %lld matvecs\n", ret, primme.initSize,
         (long long)primme.stats.numOuterIterations, (long long)primme.stats.numMatvecs);
   /* the continuum levels (i + j + 1) omega in the matrix's units: 2 w times 1, 2, 2, 3, 3, 3 */
   static const int level[6] = {1, 2, 2, 3, 3, 3};
   for (int k = 0; k < primme.initSize; k++)
      printf("eval[%d] = %.14e   |r| = %.2e   continuum 2 w (i + j + 1) = %.6f\n", k, evals[k], rnorms[k], 2.0 * w * level[k]);

   hipk_free(ctx, evecs_dev);
   primme_free(&primme);
   primme_amd_operator_destroy(op);
   hipk_csr_destroy(A);
   hipk_ctx_destroy(ctx);
   free(rp); free(ci); free(va);
   return bad;
}
