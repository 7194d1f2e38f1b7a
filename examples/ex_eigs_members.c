/* ex_eigs_members.c — the parameter block driven the way a language binding drives it: every option is looked up BY NAME
 * (primme_member_info), converted by the kind the library reports and stored with primme_set_member; enumerators come from
 * primme_constant_info.  The program includes primme.h only, prints the configuration with primme_display_params and
 * computes the 5 smallest eigenvalues of the 1-D Laplacian of order 100 with host callbacks through dprimme().
 *
 *   make -C examples && examples/ex_eigs_members   (exit code 0 = eigenvalues match 2 - 2cos(k pi/(n+1)))
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include "primme.h"

/* y = tridiag(-1, 2, -1) x for a block of host vectors */
static void laplacian_matvec(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy, int *blockSize,
      primme_params *primme, int *ierr) {
   const PRIMME_INT n = primme->n;
   for (int c = 0; c < *blockSize; c++) {
      const double *xv = (const double *)x + *ldx * c;
      double *yv = (double *)y + *ldy * c;
      for (PRIMME_INT i = 0; i < n; i++)
         yv[i] = 2.0 * xv[i] - (i > 0 ? xv[i - 1] : 0.0) - (i + 1 < n ? xv[i + 1] : 0.0);
   }
   *ierr = 0;
}

/* option = text, as it would come from a configuration file: a number, or the name of an enumerator */
static int set_by_name(primme_params *primme, const char *name, const char *text) {
   primme_params_label label = PRIMME_invalid_label;
   primme_type type;
   int arity;
   if (primme_member_info(&label, &name, &type, &arity) || arity != 1) return 1;
   if (type == primme_double) {
      double v = strtod(text, NULL);
      return primme_set_member(primme, label, &v);
   }
   if (type == primme_int) {
      int constant;
      PRIMME_INT v = primme_constant_info(text, &constant) == 0 ? constant : strtoll(text, NULL, 10);
      return primme_set_member(primme, label, &v);
   }
   return 1;
}

int main(void) {
   static const char *options[][2] = {{"n", "100"}, {"numEvals", "5"}, {"eps", "1e-9"}, {"target", "primme_smallest"},
                                      {"maxBasisSize", "20"}, {"printLevel", "0"}};
   primme_params primme;
   primme_initialize(&primme);
   for (size_t i = 0; i < sizeof(options) / sizeof(options[0]); i++)
      if (set_by_name(&primme, options[i][0], options[i][1])) {
         fprintf(stderr, "cannot set %s = %s\n", options[i][0], options[i][1]);
         return 2;
      }
   primme.matrixMatvec = laplacian_matvec;
   primme_set_method(PRIMME_DEFAULT_MIN_MATVECS, &primme);
   primme_display_params(primme);

   const int n = (int)primme.n, nev = primme.numEvals;
   double *evals = (double *)calloc((size_t)nev, sizeof(double)), *rnorms = (double *)calloc((size_t)nev, sizeof(double));
   double *evecs = (double *)calloc((size_t)n * nev, sizeof(double));   /* HOST */
   const int ret = dprimme(evals, evecs, rnorms, &primme);

   int bad = (ret != 0 || primme.initSize != nev);
   printf("dprimme returned %d: %d pairs, %" PRIMME_INT_P " outer iterations, %" PRIMME_INT_P " matvecs, %" PRIMME_INT_P " restarts\n",
         ret, primme.initSize, primme.stats.numOuterIterations, primme.stats.numMatvecs, primme.stats.numRestarts);
   const double pi = 3.14159265358979323846;
   for (int k = 0; k < nev && ret == 0; k++) {
      const double exact = 2.0 - 2.0 * cos((k + 1) * pi / (n + 1));
      printf("Eval[%d] = %.15e  error %.1e  rnorm %.1e\n", k + 1, evals[k], fabs(evals[k] - exact), rnorms[k]);
      if (fabs(evals[k] - exact) > primme.eps * primme.aNorm) bad = 1;
   }
   free(evals); free(rnorms); free(evecs);
   return bad;
}
