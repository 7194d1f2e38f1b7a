/* eigs_jd.c — JDQMR: block symmetric QMR on the projected correction equation
 *       (I - Q Q')(I - x x')(A - sigma I) t = -r,     t ⟂ [Q x]
 * with adaptive stopping driven by recurrences for the updated Ritz value and
 * eigen-residual.
 *
 *   pa_inner_solve            <- reference src/eigs/inner_solve.c:132-669
 *   apply_projected_matrix    <- reference :838-891
 *   apply_skew_projector      <- reference :769-808  (orthogonal projectors only here)
 *   apply_projected_precond   <- reference :714-741
 *   projector set-up          <- reference src/eigs/correction.c:862-997
 *
 * All n-length work is on the device: per QMR iteration one block SpMM, the projector
 * panels (hipk_panel_dots / hipk_panel_project), pairwise dot products for the b scalar
 * recurrences and one fused pass for delta/sol/|sol|^2.  The scalar recurrences and the
 * stopping logic stay on the host, restated literally.
 * Indexing note: the scalar recurrences are kept per ORIGINAL block column (index pm[i]) and
 * every panel is permuted once when columns leave the block.  The reference writes some of
 * them by position and reads them by original index (sigma_prev, Theta, rho: inner_solve.c:317,
 * :373-377, :616-620) and permutes x twice when it is also a projector (:363-366); for block
 * size 1 — where both versions coincide exactly — this does not matter, for b > 1 this file
 * implements the consistent variant and parity is asserted on the converged results.
 * Covered: the JDQMR / JDQMR_ETol presets (LeftQ iff preconditioning, LeftX, no right
 * projectors) plus orthogonal right projectors; skew projectors (K^-1-weighted, presets
 * JDQR / JD_Olsen) return PRIMME_FUNCTION_UNAVAILABLE.
 */
#include "eigs_solver.h"
#include "primme_amd_comm.h"
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

/* The QMR recurrences are REAL for complex data too (the reference takes real parts: Num_dist_dots_real,
 * inner_solve.c:283-420, and real axpy factors): on a complex panel those steps are the real kernels on the panel seen as
 * 2m reals (Re(x^H y) = the real inner product of the two 2m-vectors).  Only the operator and the projectors work with
 * complex coefficients.  RDT / RM / R2: dtype, row count and leading dimension of that real view. */
#if PA_IS_COMPLEX
#define RDT(s) ((s)->dt == HIPK_C64 ? HIPK_F64 : HIPK_F32)
#define RM(s) (2 * (s)->m)
#define R2(ld) (2 * (ld))
#else
#define RDT(s) ((s)->dt)
#define RM(s) ((s)->m)
#define R2(ld) (ld)
#endif

static int conv_test(pa_solver *s, double eval, double rnorm, int *isconv) {
   primme_params *p = s->p;
   if (p->convTestFun == pa_conv_test_absolute) {
      *isconv = rnorm < PA_MAX(p->eps, s->mach_eps * 2) * pa_problem_norm(0, p);
      return 0;
   }
   return pa_call_conv_test(p, eval, NULL, rnorm, isconv);
}

/* v(:, 0:nb) <- (I - Qhat Q') v for a panel Q (numCols columns), orthogonal form */
static int project_panel(pa_solver *s, char *Q, int64_t ldQ, char *Qhat, int64_t ldQhat, int numCols,
      char *v, int64_t ldv, int nb) {
   if (numCols <= 0 || nb <= 0) return 0;
   double t0 = pa_wtime();
   hipk_seg sq = {Q, ldQ, numCols}, sh = {Qhat, ldQhat, numCols};
   CHK(hipk_panel_dots(s->ctx, s->dt, s->m, &sq, 1, v, ldv, nb, s->d_red, numCols));
   CHK(pa_reduce(s, s->d_red, SD * numCols * nb, 1, 1));
   CHK(hipk_panel_project(s->ctx, s->dt, s->m, &sh, 1, s->d_red, numCols, v, ldv, nb, NULL));
   s->p->stats.numOrthoInnerProds += (double)numCols * nb;
   s->p->stats.timeOrtho += pa_wtime() - t0;
   return 0;
}

/* v_i <- (I - xhat_i x_i') v_i for every column i */
static int project_each(pa_solver *s, char *X, int64_t ldX, char *Xhat, int64_t ldXhat, char *v, int64_t ldv, int nb) {
   if (nb <= 0) return 0;
   double t0 = pa_wtime();
   CHK(hipk_pair_dots(s->ctx, s->dt, s->m, X, ldX, v, ldv, nb, s->d_red));
   CHK(pa_reduce(s, s->d_red, SD * nb, 0, 0));
   HS alpha[64];
   for (int i = 0; i < nb; i++) alpha[i] = -((const HS *)s->h_red)[i];
   CHK(hipk_axpy_cols(s->ctx, s->dt, s->m, (const double *)alpha, Xhat, ldXhat, v, ldv, nb));
   s->p->stats.numOrthoInnerProds += nb;
   s->p->stats.timeOrtho += pa_wtime() - t0;
   return 0;
}

/* out[c] = Re(X(:,c)^H Y(:,c)) */
static int pair_dots_host(pa_solver *s, char *X, int64_t ldX, char *Y, int64_t ldY, int nb, double *out) {
   CHK(hipk_pair_dots(s->ctx, RDT(s), RM(s), X, R2(ldX), Y, R2(ldY), nb, s->d_red));
   CHK(pa_reduce(s, s->d_red, nb, 0, 0));
   for (int i = 0; i < nb; i++) out[i] = s->h_red[i];
   return 0;
}

/* in-place column permutation of a device panel through the scratch panel T */
static int permute_panel(pa_solver *s, char *base, int64_t ldb, int n, const int *perm) {
   int moved = 0;
   for (int i = 0; i < n; i++) if (perm[i] != i) moved = 1;
   if (!moved || !base) return 0;
   /* only the tail that actually moves: one gather launch into the scratch panel and one copy back
    * (a column converging out of a block of 8 used to cost nine rectangular copies per panel) */
   int first = 0;
   while (first < n && perm[first] == first) first++;
   const int cnt = n - first;
   if (cnt > s->nT) return PRIMME_UNEXPECTED_FAILURE;
   int rel[64];
   if (cnt > 64) return PRIMME_FUNCTION_UNAVAILABLE;
   for (int i = 0; i < cnt; i++) rel[i] = perm[first + i] - first;
   for (int i = 0; i < cnt; i++) if (rel[i] < 0) return PRIMME_UNEXPECTED_FAILURE;   /* a permutation never reaches back over fixed points */
   CHK(hipk_gather_cols(s->ctx, s->dt, s->m, PCOL(s, base, ldb, first), ldb, rel, cnt, s->T, s->ld));
   CHK(hipk_copy_cols(s->ctx, s->dt, s->m, s->T, s->ld, PCOL(s, base, ldb, first), ldb, cnt));
   return 0;
}

/* swap `val` into position `pos` of the permutation (reference inner_solve.c:913-925) */
static void perm_set_value_on_pos(int *p, int val, int pos, int n) {
   for (int i = 0; i < n; i++)
      if (p[i] == val) { p[i] = p[pos]; p[pos] = val; return; }
}

typedef struct {
   char *LQ, *LX; int64_t ldLQ, ldLX; int nLQ, nLX;   /* left projectors I - LBQ LQ', I - LBX_i LX_i' ... */
   char *LBQ, *LBX; int64_t ldLBQ, ldLBX;             /* ... with LBQ = B Q, LBX = B x (B = I: the same panels) */
   char *Bx;               /* B x of a generalised problem (NULL otherwise): permuted with x when columns leave the block */
   char *Bv;               /* scratch panel for B v (generalised problems) */
   char *RQ, *RX; int64_t ldRQ, ldRX; int nRQ, nRX;   /* right projectors: I - RQ M^-1 Q', I - RX_i x_i'/xKx_i */
   int skewQ, skewX;       /* RQ = K^-1 Q with M = Q'K^-1 Q factorised; RX = K^-1 x with xKx = x'K^-1 x */
   char *x;                /* the Ritz vectors (dotted against in the X projector) */
   HS xKx[64];             /* x_i' K^-1 x_i: complex for a non-Hermitian preconditioner (reference: HSCALAR xKinvBx) */
} jd_proj;

/* ---- M = evecs' evecsHat: dense LU with partial pivoting on the host (the reference keeps a
 * Bunch-Kaufman factorisation, factorize.c:183-262; same solution up to rounding) ---- */
static int lu_factor(const HS *A, int ldA, int n, HS *LU, int *piv) {
   for (int j = 0; j < n; j++) for (int i = 0; i < n; i++) LU[i + (size_t)j * n] = A[i + (size_t)j * ldA];
   for (int k = 0; k < n; k++) {
      int pi = k;
      for (int i = k + 1; i < n; i++) if (HS_ABS(LU[i + (size_t)k * n]) > HS_ABS(LU[pi + (size_t)k * n])) pi = i;
      piv[k] = pi;
      if (LU[pi + (size_t)k * n] == 0.0) return PRIMME_LAPACK_FAILURE;
      if (pi != k) for (int j = 0; j < n; j++) { HS t = LU[k + (size_t)j * n]; LU[k + (size_t)j * n] = LU[pi + (size_t)j * n]; LU[pi + (size_t)j * n] = t; }
      for (int i = k + 1; i < n; i++) {
         const HS l = LU[i + (size_t)k * n] /= LU[k + (size_t)k * n];
         for (int j = k + 1; j < n; j++) LU[i + (size_t)j * n] -= l * LU[k + (size_t)j * n];
      }
   }
   return 0;
}
static void lu_solve(const HS *LU, const int *piv, int n, HS *b) {
   for (int k = 0; k < n; k++) { const int pi = piv[k]; if (pi != k) { HS t = b[k]; b[k] = b[pi]; b[pi] = t; } }
   for (int i = 0; i < n; i++) for (int j = 0; j < i; j++) b[i] -= LU[i + (size_t)j * n] * b[j];
   for (int i = n - 1; i >= 0; i--) { for (int j = i + 1; j < n; j++) b[i] -= LU[i + (size_t)j * n] * b[j]; b[i] /= LU[i + (size_t)i * n]; }
}

/* evecsHat(:, c0:c0+count) = K^-1 evecs(:, c0:c0+count); M and its factors extended accordingly
 * (reference restart.c:1471-1531, init.c:152-169, factorize.c:183-262).  Column indices include
 * the orthogonality constraints. */
static int extend_evecs_hat(pa_solver *s, int c0, int count) {
   if (count <= 0) return 0;
   char *src = ECOL(s, c0);
   if (s->Bevecs && !s->ref_soft_alias) {
      /* generalised problem: evecsHat = K^-1 B evecs (init.c:162-164, restart.c:1511-1515); B evecs itself is the left projector's */
      src = s->Bevecs + (size_t)c0 * s->ldevecs * s->es;
      CHK(pa_apply_B(s, ECOL(s, c0), s->ldevecs, src, s->ldevecs, count));
      s->nBevecs = c0 + count;
   }
   if (!s->evecsHat) return 0;
   char *hat = s->evecsHat + (size_t)c0 * s->ldevecs * s->es;
   CHK(pa_precond(s, src, s->ldevecs, hat, s->ldevecs, count));
   const int nM = c0 + count;
   for (int j0 = 0; j0 < count; j0 += 8) {
      const int nj = PA_MIN(8, count - j0);
      hipk_seg sq = {s->evecs, s->ldevecs, nM};
      CHK(hipk_panel_dots(s->ctx, s->dt, s->m, &sq, 1, hat + (size_t)j0 * s->ldevecs * s->es, s->ldevecs, nj, s->d_red, nM));
      CHK(pa_reduce(s, s->d_red, SD * nM * nj, 0, 0));
      for (int j = 0; j < nj; j++)
         for (int i = 0; i < nM; i++) {
            const HS mij = ((const HS *)s->h_red)[i + (size_t)j * nM];
            s->Mq[i + (size_t)(c0 + j0 + j) * s->ldM] = mij;
            if (i < c0 && !s->B) s->Mq[(c0 + j0 + j) + (size_t)i * s->ldM] = HS_CONJ(mij);   /* K Hermitian */
         }
   }
   /* M = evecs' K^-1 B evecs is not Hermitian (factorize.c:190-195): the rows of the new vectors against the old K^-1 B evecs */
   if (s->B) for (int i0 = 0; i0 < c0; i0 += 8) {
      const int ni = PA_MIN(8, c0 - i0);
      hipk_seg sq = {ECOL(s, c0), s->ldevecs, count};
      CHK(hipk_panel_dots(s->ctx, s->dt, s->m, &sq, 1, s->evecsHat + (size_t)i0 * s->ldevecs * s->es, s->ldevecs, ni, s->d_red, count));
      CHK(pa_reduce(s, s->d_red, SD * count * ni, 0, 0));
      for (int i = 0; i < ni; i++)
         for (int j = 0; j < count; j++) s->Mq[(c0 + j) + (size_t)(i0 + i) * s->ldM] = ((const HS *)s->h_red)[j + (size_t)i * count];
   }
   return lu_factor(s->Mq, s->ldM, nM, s->Mlu, s->Mpiv);
}

int pa_evecs_hat_init(pa_solver *s) {
   if (!s->evecsHat && !s->Bevecs) return 0;
   s->p->ShiftsForPreconditioner = NULL;
   return extend_evecs_hat(s, 0, s->p->numOrthoConst);
}

/* after a restart: K^-1 of the vectors that converged since the last call */
int pa_evecs_hat_update(pa_solver *s, int *numConvergedStored, int numConverged) {
   primme_params *p = s->p;
   if (!s->evecsHat) return 0;
   if (!p->locking) *numConvergedStored = 0;
   const int stored = *numConvergedStored, recent = numConverged - stored;
   double *shifts = NULL;
   int own = 0;
   if (numConverged <= p->numTargetShifts) shifts = &p->targetShifts[stored];
   else if (p->numTargetShifts > 0) {
      shifts = (double *)malloc(sizeof(double) * (size_t)(numConverged > 0 ? numConverged : 1));
      if (!shifts) return PRIMME_MALLOC_FAILURE;
      own = 1;
      for (int i = 0; i < recent; i++) shifts[i] = p->targetShifts[PA_MIN(i + stored, p->numTargetShifts - 1)];
   }
   p->ShiftsForPreconditioner = shifts;
   int rc = extend_evecs_hat(s, p->numOrthoConst + stored, recent);
   p->ShiftsForPreconditioner = NULL;
   if (own) free(shifts);
   if (rc) return rc;
   *numConvergedStored = numConverged;
   return 0;
}

/* v <- (I - Qhat M^-1 Q') v: overlaps on the device, the small solve on the host */
static int skew_project_Q(pa_solver *s, const jd_proj *P, char *v, int64_t ldv, int nb) {
   const int nQ = P->nRQ;
   if (nQ <= 0 || nb <= 0) return 0;
   double t0 = pa_wtime();
   hipk_seg sq = {s->evecs, s->ldevecs, nQ}, sh = {P->RQ, P->ldRQ, nQ};
   CHK(hipk_panel_dots(s->ctx, s->dt, s->m, &sq, 1, v, ldv, nb, s->d_red, nQ));
   CHK(pa_reduce(s, s->d_red, SD * nQ * nb, 0, 0));
   if (nQ > 1) for (int c = 0; c < nb; c++) lu_solve(s->Mlu, s->Mpiv, nQ, (HS *)s->h_red + (size_t)c * nQ);
   else for (int c = 0; c < nb; c++) ((HS *)s->h_red)[c] /= s->Mq[0];
   CHK(hipk_h2d(s->ctx, s->d_red, s->h_red, sizeof(HS) * (size_t)nQ * nb));
   CHK(hipk_panel_project(s->ctx, s->dt, s->m, &sh, 1, s->d_red, nQ, v, ldv, nb, NULL));
   s->p->stats.numOrthoInnerProds += (double)nQ * nb;
   s->p->stats.timeOrtho += pa_wtime() - t0;
   return 0;
}

static int jd_no_project_triple(void) {           /* A/B knob, read once */
   static int v = -1;
   if (v < 0) v = getenv("PRIMME_AMD_NO_PROJECT_TRIPLE") != NULL;
   return v;
}

/* result = (I - Q Q')(I - x x')... (A - shift) v, and vdot[c] = v_c' result_c.  The axpy of every
 * step is fused with the dot product that follows it (hipk_axpy_dot): same arithmetic as the
 * reference's separate Num_axpy / Num_dist_dots calls, two passes over the panels fewer. */
/* xr_out != NULL (blocks): the projection against x is NOT applied to `result`; xr_out[c] = x_c' result_c and
 * vdot[c] = v'(I - x x') result = v'result - (x'result)(v'x) come from one pass of three inner products
 * (hipk_triple_dots), and the caller folds the projection into its update of g (hipk_axpy_proj_dot). */
/* nowait (with xr_out): the three inner products stay in HBM (s->d_red[0 .. 3 nb), mirrored), nothing is waited for and
 * vdot / xr_out are NOT set: the launches of the one-synchronisation step read them on the device (inner_solve) */
static int apply_projected_matrix(pa_solver *s, char *v, int64_t ldv, const double *shift, const jd_proj *P,
      int nb, char *result, int64_t ldres, double *vdot, double *xr_out, int nowait) {
   /* result = A v - shift v: in ONE launch when the operator is the library's own CSR matrix (the shift is
    * applied in the SpMM epilogue), otherwise the callback followed by an axpy */
   int shifted = 0;
   if (nb > 1 && !s->B && s->p->matrixMatvec == primme_amd_matvec && s->p->matrix) {
      double t0 = pa_wtime();
      const int rcs = primme_amd_operator_apply_shifted((primme_amd_operator *)s->p->matrix, hipk_ctx_stream(s->ctx), v, ldv,
            result, ldres, nb, shift);
      if (rcs < 0) return rcs;
      if (rcs == 0) {
         shifted = 1;
         if (s->phase_timing) CHK(hipk_sync(s->ctx));
         s->p->stats.timeMatvec += pa_wtime() - t0;
         s->p->stats.numMatvecs += nb;
      }
   }
   if (!shifted) CHK(pa_matvec(s, v, ldv, result, ldres, 0, nb));
   /* generalised problem: result = A v - shift B v, left projectors I - (B Q) Q' and I - (B x) x' (inner_solve.c:838-890) */
   char *av = v;
   int64_t ldav = ldv;
   if (s->B) {
      if (xr_out) return PRIMME_UNEXPECTED_FAILURE;      /* the folded x-projection is the standard problem's */
      CHK(pa_apply_B(s, v, ldv, P->Bv, s->ld, nb));
      av = P->Bv; ldav = s->ld;
   }
   double ms[64];
   for (int i = 0; i < nb; i++) ms[i] = -shift[i];
   if (P->nLX > 0) {
      double t0 = pa_wtime();
#if PA_IS_COMPLEX
      /* the reference's operation order with complex projector coefficients: result -= shift v (real), (I - Q Q^H),
       * c = x^H result (complex), result -= c x, vdot = Re(v^H result) */
      (void)xr_out;
      if (!shifted) CHK(hipk_axpy_cols(s->ctx, RDT(s), RM(s), ms, av, R2(ldav), result, R2(ldres), nb));
      if (P->nLQ > 0) CHK(project_panel(s, P->LQ, P->ldLQ, P->LBQ, P->ldLBQ, P->nLQ, result, ldres, nb));
      CHK(hipk_pair_dots(s->ctx, s->dt, s->m, P->LX, P->ldLX, result, ldres, nb, s->d_red));
      CHK(pa_reduce(s, s->d_red, SD * nb, 0, 0));
      {
         HS mc[64];
         for (int i = 0; i < nb; i++) mc[i] = -((const HS *)s->h_red)[i];
         CHK(hipk_axpy_cols(s->ctx, s->dt, s->m, (const double *)mc, P->LBX, P->ldLBX, result, ldres, nb));
      }
      CHK(pair_dots_host(s, v, ldv, result, ldres, nb, vdot));
      s->p->stats.numOrthoInnerProds += nb;
      s->p->stats.timeOrtho += pa_wtime() - t0;
      return 0;
#else
      if (xr_out) {
         if (!shifted) CHK(hipk_axpy_cols(s->ctx, s->dt, s->m, ms, v, ldv, result, ldres, nb));
         /* the projection against the locked vectors and the three inner products of the step in ONE pass over the panel
          * (hipk_project_triple_dots: the arithmetic of the two launches, bit for bit; PRIMME_AMD_NO_PROJECT_TRIPLE=1 keeps them) */
         int fused_pt = 0;
         if (P->nLQ > 0 && !jd_no_project_triple()) {
            double tq = pa_wtime();
            hipk_seg sq = {P->LQ, P->ldLQ, P->nLQ};
            CHK(hipk_panel_dots(s->ctx, s->dt, s->m, &sq, 1, result, ldres, nb, s->d_red + 3 * 64, P->nLQ));
            CHK(pa_reduce(s, s->d_red + 3 * 64, P->nLQ * nb, 1, 1));
            const int rcp = hipk_project_triple_dots(s->ctx, s->dt, s->m, &sq, 1, s->d_red + 3 * 64, P->nLQ, result, ldres, nb, P->LX, P->ldLX, v, ldv, s->d_red);
            if (rcp < 0) return rcp;
            if (rcp == 0) { fused_pt = 1; s->p->stats.numOrthoInnerProds += (double)P->nLQ * nb; }
            else CHK(hipk_panel_project(s->ctx, s->dt, s->m, &sq, 1, s->d_red + 3 * 64, P->nLQ, result, ldres, nb, NULL));
            s->p->stats.timeOrtho += pa_wtime() - tq;
            if (rcp != 0) { s->p->stats.numOrthoInnerProds += (double)P->nLQ * nb; }
         } else if (P->nLQ > 0) CHK(project_panel(s, P->LQ, P->ldLQ, P->LQ, P->ldLQ, P->nLQ, result, ldres, nb));
         if (!fused_pt) CHK(hipk_triple_dots(s->ctx, s->dt, s->m, P->LX, P->ldLX, v, ldv, result, ldres, nb, s->d_red));
         if (nowait) {
            CHK(pa_reduce(s, s->d_red, 3 * nb, 1, 1));
            s->p->stats.numOrthoInnerProds += 3 * nb;
            s->p->stats.timeOrtho += pa_wtime() - t0;
            return 0;
         }
         CHK(pa_reduce(s, s->d_red, 3 * nb, 0, 0));
         for (int i = 0; i < nb; i++) {
            xr_out[i] = s->h_red[i];
            vdot[i] = s->h_red[nb + i] - s->h_red[i] * s->h_red[2 * nb + i];
         }
         s->p->stats.numOrthoInnerProds += 3 * nb;
         s->p->stats.timeOrtho += pa_wtime() - t0;
         return 0;
      }
      if (P->nLQ > 0) {
         if (!shifted) CHK(hipk_axpy_cols(s->ctx, s->dt, s->m, ms, av, ldav, result, ldres, nb));
         CHK(project_panel(s, P->LQ, P->ldLQ, P->LBQ, P->ldLBQ, P->nLQ, result, ldres, nb));
         CHK(hipk_pair_dots(s->ctx, s->dt, s->m, P->LX, P->ldLX, result, ldres, nb, s->d_red));
      } else if (shifted) {
         CHK(hipk_pair_dots(s->ctx, s->dt, s->m, P->LX, P->ldLX, result, ldres, nb, s->d_red));
      } else {
         /* result -= shift v  and  x' result */
         CHK(hipk_axpy_dot(s->ctx, s->dt, s->m, nb, ms, av, ldav, result, ldres, P->LX, P->ldLX, s->d_red));
      }
      CHK(pa_reduce(s, s->d_red, nb, 0, 0));
      double ma[64];
      for (int i = 0; i < nb; i++) ma[i] = -s->h_red[i];
      /* result -= (x' result) B x  and  v' result */
      CHK(hipk_axpy_dot(s->ctx, s->dt, s->m, nb, ma, P->LBX, P->ldLBX, result, ldres, v, ldv, s->d_red));
      CHK(pa_reduce(s, s->d_red, nb, 0, 0));
      for (int i = 0; i < nb; i++) vdot[i] = s->h_red[i];
      s->p->stats.numOrthoInnerProds += nb;
      s->p->stats.timeOrtho += pa_wtime() - t0;
#endif
   } else {
      if (!shifted) CHK(hipk_axpy_cols(s->ctx, RDT(s), RM(s), ms, av, R2(ldav), result, R2(ldres), nb));
      CHK(project_panel(s, P->LQ, P->ldLQ, P->LBQ, P->ldLBQ, P->nLQ, result, ldres, nb));
      CHK(pair_dots_host(s, v, ldv, result, ldres, nb, vdot));
   }
   return 0;
}

static int apply_projected_preconditioner(pa_solver *s, char *v, int64_t ldv, const jd_proj *P, int nb,
      char *result, int64_t ldres) {
   CHK(pa_precond(s, v, ldv, result, ldres, nb));
   if (P->skewQ) CHK(skew_project_Q(s, P, result, ldres, nb));
   else CHK(project_panel(s, s->evecs, s->ldevecs, P->RQ, P->ldRQ, P->nRQ, result, ldres, nb));
   if (P->nRX > 0) {
      if (P->skewX) {
         /* result_i -= K^-1 x_i (x_i' result_i) / (x_i' K^-1 x_i)  (reference inner_solve.c:737-741) */
         double t0 = pa_wtime();
         CHK(hipk_pair_dots(s->ctx, s->dt, s->m, P->x, s->ld, result, ldres, nb, s->d_red));
         CHK(pa_reduce(s, s->d_red, SD * nb, 0, 0));
         HS alpha[64];
         for (int i = 0; i < nb; i++) alpha[i] = -((const HS *)s->h_red)[i] / P->xKx[i];
         CHK(hipk_axpy_cols(s->ctx, s->dt, s->m, (const double *)alpha, P->RX, P->ldRX, result, ldres, nb));
         s->p->stats.numOrthoInnerProds += nb;
         s->p->stats.timeOrtho += pa_wtime() - t0;
      } else {
         CHK(project_each(s, P->x, s->ld, P->RX, P->ldRX, result, ldres, nb));      /* (I - (B x) x'): RX = B x, = x for B = I */
      }
   }
   return 0;
}

/* Block QMR.  x, r: the block's Ritz vectors and residuals (V / W slots at basisSize);
 * sol receives the corrections.  eval[i], shift[i], rnorm[i] per block vector. */
static int inner_solve(pa_solver *s, int blockSize, char *x, char *r, const double *rnorm, jd_proj *P,
      char *sol, const double *eval, double *shift, int *touch) {
   primme_params *p = s->p;
   const int64_t ld = s->ld;
   const int b0 = blockSize;
   char *g = s->Jw, *d = PCOL(s, s->Jw, ld, b0), *delta = PCOL(s, s->Jw, ld, 2 * b0), *w = PCOL(s, s->Jw, ld, 3 * b0);
   double sigma_prev[64], rho_prev[64], rho[64], alpha_prev[64], Theta_prev[64], Theta[64], tau_init[64],
         tau_prev[64], tau[64], Beta_prev[64], Delta_prev[64], Psi_prev[64], eta[64], eval_prev[64],
         eres_updated[64], Gamma_prev[64], Phi_prev[64], gamma[64], dot_sol[64], tmp[64], gg[64];
   /* without preconditioner and right projectors the "preconditioned" vector is g itself: no
    * copy, and rho = g'g is the dot product already taken for Theta */
   const int plain_K = (!p->correctionParams.precondition && P->nRQ == 0 && P->nRX == 0);
   /* block runs with the library's own Jacobi preconditioner and no right projectors: the QMR update, the
    * next K^-1 g and the two reductions they need are ONE pass (hipk_qmr_update_jacobi) */
   const void *jac_diag = NULL;
   int jac_fixed = 0;
   double jac_shift = 0.0, rho_new[64];
   const int fuse_pk = (!PA_IS_COMPLEX && b0 > 1 && !plain_K && !s->B && getenv("PRIMME_AMD_JDQMR_REF_INDEXING") == NULL && p->correctionParams.precondition && p->applyPreconditioner == primme_amd_jacobi_precond &&
                        p->preconditioner && P->nRQ == 0 && P->nRX == 0 && !P->skewQ &&
                        primme_amd_operator_jacobi_data((primme_amd_operator *)p->preconditioner, &jac_diag, &jac_fixed, &jac_shift) == 0);
   /* ... and with the x-projection folded into the update of g (fold_x) the inner product rho = g'K^-1 g of the NEXT step
    * rides on that update (hipk_axpy_proj_dot_jacobi): beta is known one synchronisation earlier, and the QMR update
    * writes the new direction d = K^-1 g + beta d in place (hipk_qmr_update_dir) — w = K^-1 g is never stored and the
    * separate pass w += beta d disappears (7 array passes per column instead of 11 after the update of g).
    * PRIMME_AMD_NO_EARLY_RHO=1 keeps the round-2 sequence (A/B knob). */
   static int no_early = -1;
   if (no_early < 0) no_early = getenv("PRIMME_AMD_NO_EARLY_RHO") != NULL;
   /* PRIMME_AMD_JDQMR_REF_INDEXING=1 (blocks): restate the reference's own indexing of the block recurrences, quirks included —
    * sigma_prev, Theta and rho are WRITTEN by block position (Num_dist_dots_real fills [0, blockSize)) but READ by original
    * column (inner_solve.c:317, :329-337, :373-377, :616-620), and x is permuted once more for every projector it doubles as
    * (:352-357, :600-603) — in the reference's operation order (no folded x-projection, no early rho, three waits).  As long as
    * no column has left the block both indexings coincide; afterwards this mode follows the reference's history where the
    * default keeps every recurrence with its own column.  A parity instrument, not a fast path. */
   const int ref_ix = (b0 > 1 && getenv("PRIMME_AMD_JDQMR_REF_INDEXING") != NULL);
   const int early_rho = fuse_pk && P->nLX > 0 && !no_early && !ref_ix;
   int pm[64], p0[64];
   const int three_waits = getenv("PRIMME_AMD_QMR_THREE_WAITS") != NULL;      /* (A/B knob, read once per inner solve: tests switch it within a process) */
   const int adaptive = (p->correctionParams.convTest == primme_adaptive ||
                         p->correctionParams.convTest == primme_adaptive_ETolerance);
   int i, isConv;
   if (blockSize > 64) return PRIMME_FUNCTION_UNAVAILABLE;   /* inner solves with more than 64 right-hand sides */

   for (i = 0; i < blockSize; i++) tau_prev[i] = tau_init[i] = rnorm[i];
   double LTolerance = s->mach_eps * pa_problem_norm(1, p), LTolerance_factor = 1.0, ETolerance = 0.0,
          ETolerance_factor = 0.0;
   switch (p->correctionParams.convTest) {
   case primme_full_LTolerance: break;
   case primme_decreasing_LTolerance:
      LTolerance = PA_MAX(LTolerance, pow(p->correctionParams.relTolBase, -(double)*touch));
      (*touch)++;
      break;
   case primme_adaptive:
      LTolerance_factor = ETolerance_factor = pow(1.8, -(double)*touch);
      break;
   case primme_adaptive_ETolerance:
      LTolerance_factor = ETolerance_factor = pow(1.8, -(double)*touch);
      ETolerance = 0.1;
      break;
   }
   int64_t maxIterations = (p->maxMatvecs > 0) ? p->maxMatvecs - p->stats.numMatvecs : INT_MAX;
   if (p->correctionParams.maxInnerIterations > 0)
      maxIterations = PA_MIN((int64_t)p->correctionParams.maxInnerIterations, maxIterations);

   /* zero initial guess: g = r, d = K^-1 g (projected) */
   CHK(hipk_copy_cols(s->ctx, s->dt, s->m, r, ld, g, ld, blockSize));
   CHK(apply_projected_preconditioner(s, g, ld, P, blockSize, d, ld));
   for (i = 0; i < blockSize; i++) { Theta_prev[i] = 0.0; eval_prev[i] = eval[i]; }
   CHK(pair_dots_host(s, g, ld, d, ld, blockSize, rho_prev));
   for (i = 0; i < blockSize; i++)
      Beta_prev[i] = Delta_prev[i] = Psi_prev[i] = Gamma_prev[i] = Phi_prev[i] = eres_updated[i] = 0.0;
   CHK(hipk_memset0(s->ctx, delta, (size_t)ld * s->es * blockSize));
   CHK(hipk_memset0(s->ctx, sol, (size_t)ld * s->es * blockSize));
   for (i = 0; i < blockSize; i++) pm[i] = i;
   /* generalised problem with the adaptive tests: |B x|^2 enters the estimate of the eigen-residual (inner_solve.c:296-303) */
   double normBx[64];
   for (i = 0; i < blockSize; i++) normBx[i] = 1.0;
   if (adaptive && s->B) CHK(pair_dots_host(s, P->Bx, ld, P->Bx, ld, blockSize, normBx));

   for (int64_t numIts = 0; numIts < maxIterations && blockSize > 0; numIts++) {
      /* blocks: the x-projection of w is folded into the update of g below (one pass and one
       * synchronisation fewer per step); block size 1 keeps the reference's operation order */
      const int fold_x = (!PA_IS_COMPLEX && b0 > 1 && P->nLX > 0 && !ref_ix && !s->B);
      double xr[64];
      /* ONE host synchronisation per step (round 5): with the library's Jacobi preconditioner and the folded x-projection the
       * step is three launches — (A - shift) d with its three inner products, the update of g (+ g'g, g'K^-1 g), the QMR
       * update that also writes the next direction (+ |sol|^2) — whose coefficients alpha, gamma, eta, beta are functions of the
       * reductions of the launches before them and of the previous step's rho, tau, Theta.  They are evaluated ON THE DEVICE,
       * in the prologue of the launch that applies them (hipk_axpy_proj_dot_jacobi_dev, hipk_qmr_update_dir_dev), the host
       * enqueues all three, waits ONCE and then evaluates the same expressions on the mirrored reductions (the code below,
       * unchanged) for its own bookkeeping: the stopping tests, the columns that leave the block, the next step's state.
       * Same roundings on both sides (hipk_vec.hip: qmr_alpha_dev), so the history is the three-wait sequence's, bit for bit.
       * PRIMME_AMD_QMR_THREE_WAITS=1 keeps that sequence (A/B knob).  Needs reductions that stay on the device. */
      const int onewait = !three_waits && early_rho && fold_x && numIts + 1 < maxIterations && blockSize <= 8 &&
                          !(s->parallel && !s->dev_comm) && 3 * 64 + 3 * 8 < s->red_cap;
      double gg_all[8], rho_all[8], dot_all[8];
#if !PA_IS_COMPLEX
      pa_qmr_steps[0]++;
#endif
      if (onewait) {
#if !PA_IS_COMPLEX
         pa_qmr_steps[1]++;
         double rp[8], tp[8], thp[8], jsh[8];
         double *d_tri = s->d_red, *d_ggr = s->d_red + 3 * 64, *d_dot = s->d_red + 3 * 64 + 16;
         for (i = 0; i < blockSize; i++) {
            const int q = pm[i];
            rp[i] = rho_prev[q]; tp[i] = tau_prev[q]; thp[i] = Theta_prev[q];
            jsh[i] = jac_fixed ? jac_shift : (p->ShiftsForPreconditioner ? p->ShiftsForPreconditioner[i] : 0.0);
         }
         const double md = 1e-14 * (p->aNorm >= 0.0 ? p->aNorm : 1.0);
         CHK(apply_projected_matrix(s, d, ld, shift, P, blockSize, w, ld, tmp, xr, 1));
         CHK(hipk_axpy_proj_dot_jacobi_dev(s->ctx, s->dt, s->m, blockSize, d_tri, rp, s->mach_eps, w, ld, P->LX, P->ldLX, g, ld, jac_diag, jsh, md, d_ggr));
         CHK(pa_reduce(s, d_ggr, 2 * blockSize, 1, 1));
         double t0 = pa_wtime();
         CHK(hipk_qmr_update_dir_dev(s->ctx, s->dt, s->m, blockSize, d_tri, d_ggr, rp, tp, thp, s->mach_eps, d, ld, delta, ld, sol, ld, g, ld,
               jac_diag, jsh, md, d_dot));
         CHK(pa_reduce(s, d_dot, blockSize, 0, 0));                    /* the one synchronisation of the step */
         p->stats.timePrecond += pa_wtime() - t0;
         const double *h3 = s->h_red, *hg = s->h_red + 3 * 64, *hd = s->h_red + 3 * 64 + 16;
         for (i = 0; i < blockSize; i++) {
            xr[i] = h3[i];
            tmp[i] = h3[blockSize + i] - h3[i] * h3[2 * blockSize + i];
            gg_all[i] = hg[i]; rho_all[i] = hg[blockSize + i]; dot_all[i] = hd[i];
         }
#endif
      } else
      CHK(apply_projected_matrix(s, d, ld, shift, P, blockSize, w, ld, tmp, fold_x ? xr : NULL, 0));
      for (i = 0; i < blockSize; i++) sigma_prev[ref_ix ? i : pm[i]] = tmp[i];

      int conv = 0;
      double malpha[64];
      for (i = 0; i < blockSize; i++) { p0[i] = i; malpha[i] = 0.0; }
      for (i = 0; i < blockSize; i++) {
         const int q = pm[i];
         int bad = (!isfinite(sigma_prev[q]) || sigma_prev[q] == 0.0);
         if (!bad) {
            alpha_prev[q] = rho_prev[q] / sigma_prev[q];
            bad = (!isfinite(alpha_prev[q]) || fabs(alpha_prev[q]) < s->mach_eps || fabs(alpha_prev[q]) > 1.0 / s->mach_eps);
         }
         if (bad) {
            if (numIts == 0) CHK(hipk_copy_cols(s->ctx, s->dt, s->m, PCOL(s, r, ld, i), ld, PCOL(s, sol, ld, i), ld, 1));
            perm_set_value_on_pos(p0, i, blockSize - ++conv, blockSize);
            continue;
         }
         malpha[i] = -alpha_prev[q];
      }
      /* g -= alpha w (0 for dropped columns) and g'g in the same pass */
      const int early = early_rho && fold_x && numIts + 1 < maxIterations;
      if (onewait) {
         /* the update of g ran on the device with the same alpha (0 for the columns dropped above) */
         for (i = 0; i < blockSize; i++) { gg[i] = gg_all[i]; rho_new[i] = rho_all[i]; }
      } else if (early) {
         double al[64], jsh[64];
         for (i = 0; i < blockSize; i++) {
            al[i] = -malpha[i];
            jsh[i] = jac_fixed ? jac_shift : (p->ShiftsForPreconditioner ? p->ShiftsForPreconditioner[i] : 0.0);
         }
         CHK(hipk_axpy_proj_dot_jacobi(s->ctx, s->dt, s->m, blockSize, al, xr, w, ld, P->LX, P->ldLX, g, ld, jac_diag, jsh,
               1e-14 * (p->aNorm >= 0.0 ? p->aNorm : 1.0), s->d_red));
         CHK(pa_reduce(s, s->d_red, 2 * blockSize, 0, 0));
         for (i = 0; i < blockSize; i++) { gg[i] = s->h_red[i]; rho_new[i] = s->h_red[blockSize + i]; }
      } else {
      if (fold_x) {
         double al[64];
         for (i = 0; i < blockSize; i++) al[i] = -malpha[i];
         CHK(hipk_axpy_proj_dot(s->ctx, s->dt, s->m, blockSize, al, xr, w, ld, P->LX, P->ldLX, g, ld, s->d_red));
      } else
      CHK(hipk_axpy_dot(s->ctx, RDT(s), RM(s), blockSize, malpha, w, R2(ld), g, R2(ld), NULL, 0, s->d_red));
      CHK(pa_reduce(s, s->d_red, blockSize, 0, 0));
      for (i = 0; i < blockSize; i++) gg[i] = s->h_red[i];
      }

#define SHRINK()                                                                                   \
      do {                                                                                         \
         pa_permute_ints(pm, blockSize, p0);                                                       \
         pa_permute_reals(shift, 1, blockSize, 1, p0);                                             \
         pa_permute_reals(gg, 1, blockSize, 1, p0);                                                \
         CHK(permute_panel(s, g, ld, blockSize, p0));                                              \
         CHK(permute_panel(s, d, ld, blockSize, p0));                                              \
         CHK(permute_panel(s, delta, ld, blockSize, p0));                                          \
         CHK(permute_panel(s, r, ld, blockSize, p0));                                              \
         CHK(permute_panel(s, x, ld, blockSize, p0));    /* LX / RX alias x */                     \
         if (ref_ix) {   /* the reference permutes the aliases too: once more per projector x doubles as */ \
            if (P->nLX > 0 && P->LX == x) CHK(permute_panel(s, x, ld, blockSize, p0));             \
            if (P->nRX > 0 && P->RX == x) CHK(permute_panel(s, x, ld, blockSize, p0));             \
         }                                                                                         \
         if (P->skewX && P->nRX) {                                                                 \
            CHK(permute_panel(s, P->RX, P->ldRX, blockSize, p0));                                  \
            pa_permute_cols(P->xKx, 1, blockSize, 1, p0);                                          \
         }                                                                                         \
         /* LBX / RX alias B x.  (The reference permutes B x only where it doubles as the right projector,            \
          * inner_solve.c:352-357: its left projector pairs x_i with the B x of another column once one has left) */  \
         if (P->Bx && (!ref_ix || (P->nRX > 0 && P->RX == P->Bx))) CHK(permute_panel(s, P->Bx, ld, blockSize, p0)); \
         CHK(permute_panel(s, sol, ld, blockSize, p0));                                            \
         blockSize -= conv;                                                                        \
         if (P->nLX) P->nLX -= conv;                                                               \
         if (P->nRX) P->nRX -= conv;                                                               \
      } while (0)
      if (early && conv > 0) pa_permute_reals(rho_new, 1, blockSize, 1, p0);
      if (onewait && conv > 0) pa_permute_reals(dot_all, 1, blockSize, 1, p0);
      SHRINK();
      if (blockSize <= 0) break;

      double gam_c[64], eta_c[64];
      if (ref_ix) for (i = 0; i < blockSize; i++) Theta[i] = gg[i];      /* written by position ... */
      for (i = 0; i < blockSize; i++) {
         const int q = pm[i];
         Theta[q] = sqrt(ref_ix ? Theta[q] : gg[i]) / tau_prev[q];       /* ... read by original column */
         const double c = 1.0 / sqrt(1 + Theta[q] * Theta[q]);
         tau[q] = tau_prev[q] * Theta[q] * c;
         gamma[q] = c * c * Theta_prev[q] * Theta_prev[q];
         eta[q] = alpha_prev[q] * c * c;
         gam_c[i] = gamma[q]; eta_c[i] = eta[q];
      }
      /* delta = gamma delta + eta d; sol += delta; |sol|^2 */
      int have_w = 0, have_d = 0;
      if (onewait) {
         /* the QMR update and the next direction ran on the device with the same gamma, eta, beta (evaluated there from the
          * same reductions); the columns dropped above were left alone */
         for (i = 0; i < blockSize; i++) dot_sol[i] = dot_all[i];
         p->stats.numPreconds += blockSize;
         have_d = 1;
      } else if (early) {
         /* rho of the next step is known: the update writes the next direction straight into d */
         double jsh[64], beta_c[64];
         for (i = 0; i < blockSize; i++) {
            jsh[i] = jac_fixed ? jac_shift : (p->ShiftsForPreconditioner ? p->ShiftsForPreconditioner[i] : 0.0);
            beta_c[i] = rho_new[i] / rho_prev[pm[i]];
         }
         double t0 = pa_wtime();
         CHK(hipk_qmr_update_dir(s->ctx, s->dt, s->m, blockSize, gam_c, eta_c, beta_c, d, ld, delta, ld, sol, ld, g, ld, jac_diag, jsh,
               1e-14 * (p->aNorm >= 0.0 ? p->aNorm : 1.0), s->d_red));
         CHK(pa_reduce(s, s->d_red, blockSize, 0, 0));
         for (i = 0; i < blockSize; i++) dot_sol[i] = s->h_red[i];
         p->stats.numPreconds += blockSize;
         p->stats.timePrecond += pa_wtime() - t0;
         have_d = 1;
      } else if (fuse_pk && numIts + 1 < maxIterations) {
         double jsh[64];
         for (i = 0; i < blockSize; i++) jsh[i] = jac_fixed ? jac_shift : (p->ShiftsForPreconditioner ? p->ShiftsForPreconditioner[i] : 0.0);
         double t0 = pa_wtime();
         CHK(hipk_qmr_update_jacobi(s->ctx, s->dt, s->m, blockSize, gam_c, eta_c, d, ld, delta, ld, sol, ld, g, ld, jac_diag, jsh,
               1e-14 * (p->aNorm >= 0.0 ? p->aNorm : 1.0), w, ld, s->d_red));
         CHK(pa_reduce(s, s->d_red, 2 * blockSize, 0, 0));
         for (i = 0; i < blockSize; i++) { dot_sol[i] = s->h_red[i]; rho_new[i] = s->h_red[blockSize + i]; }
         p->stats.numPreconds += blockSize;
         p->stats.timePrecond += pa_wtime() - t0;
         have_w = 1;
      } else {
         CHK(hipk_qmr_update(s->ctx, RDT(s), RM(s), blockSize, gam_c, eta_c, d, R2(ld), delta, R2(ld), sol, R2(ld), s->d_red));
         if (adaptive) {
            CHK(pa_reduce(s, s->d_red, blockSize, 0, 0));
            for (i = 0; i < blockSize; i++) dot_sol[i] = s->h_red[i];
            /* generalised problem: the B-norm of the correction, sol' B sol (inner_solve.c:416-422) */
            if (s->B) {
               CHK(pa_apply_B(s, sol, ld, P->Bv, ld, blockSize));
               CHK(pair_dots_host(s, sol, ld, P->Bv, ld, blockSize, dot_sol));
            }
         }
      }

      conv = 0;
      for (i = 0; i < blockSize; i++) p0[i] = i;
      for (i = 0; i < blockSize; i++) {
         const int q = pm[i];
         if (fabs(rho_prev[q]) == 0.0) { perm_set_value_on_pos(p0, i, blockSize - ++conv, blockSize); continue; }
         if (numIts > 0 && tau[q] < LTolerance) { perm_set_value_on_pos(p0, i, blockSize - ++conv, blockSize); continue; }
         if (ETolerance > 0.0 || ETolerance_factor > 0.0) {
            /* recurrences for the Ritz value and eigen-residual of x + sol */
            const double Delta = gamma[q] * Delta_prev[q] + eta[q] * rho_prev[q];
            const double Beta = Beta_prev[q] - Delta;
            const double Phi = gamma[q] * gamma[q] * Phi_prev[q] + eta[q] * eta[q] * sigma_prev[q];
            const double Psi = gamma[q] * Psi_prev[q] + gamma[q] * Phi_prev[q];
            const double Gamma = Gamma_prev[q] + 2.0 * Psi + Phi;
            const double nrm = 1.0 + dot_sol[i];
            const double eval_updated = shift[i] + (eval[q] - shift[i] + 2 * Beta + Gamma) / nrm;
            const double eres2 = (tau[q] * tau[q]) / nrm + (normBx[q] * (eval[q] - shift[i] + Beta) * (eval[q] - shift[i] + Beta)) / nrm -
                                 (eval_updated - shift[i]) * (eval_updated - shift[i]);
            const double eres_prev = eres_updated[q];
            eres_updated[q] = (eres2 < 0) ? sqrt((tau[q] * tau[q]) / nrm) : sqrt(eres2);
            Delta_prev[q] = Delta; Beta_prev[q] = Beta; Phi_prev[q] = Phi; Psi_prev[q] = Psi; Gamma_prev[q] = Gamma;

            if (numIts > 0 && (tau_prev[q] <= eres_updated[q] || eres_prev <= tau[q])) {
               perm_set_value_on_pos(p0, i, blockSize - ++conv, blockSize); continue;
            }
            if ((p->target == primme_smallest && eval_updated > eval_prev[q]) ||
                  (p->target == primme_largest && eval_updated < eval_prev[q]) ||
                  (p->target == primme_closest_abs && fabs(eval[q] - eval_updated) > tau_init[q] + eres_updated[q])) {
               perm_set_value_on_pos(p0, i, blockSize - ++conv, blockSize); continue;
            }
            if (numIts > 0 && eres_updated[q] < ETolerance * tau_init[q]) {
               perm_set_value_on_pos(p0, i, blockSize - ++conv, blockSize); continue;
            }
            const double tol = PA_MIN(tau[q] / LTolerance_factor, eres_updated[q] / ETolerance_factor);
            CHK(conv_test(s, eval_updated, tol, &isConv));
            if (numIts > 0 && isConv) {
               (*touch)++;
               perm_set_value_on_pos(p0, i, blockSize - ++conv, blockSize); continue;
            }
            eval_prev[q] = eval_updated;
            if (p->monitorFun || p->printLevel >= 4) {      /* report of the inner step (inner_solve.c:550-558) */
               p->stats.elapsedTime = pa_wtime() - s->startTime;
               CHK(pa_call_monitor_inner(p, eval_updated, eres_updated[q], -1, (int)numIts, tau[q]));
            }
         } else {
            CHK(conv_test(s, eval[q], tau[q] / LTolerance_factor * sqrt((double)numIts), &isConv));
            if (numIts > 0 && isConv) { perm_set_value_on_pos(p0, i, blockSize - ++conv, blockSize); continue; }
            if (p->monitorFun || p->printLevel >= 4) {      /* (inner_solve.c:581-588) */
               p->stats.elapsedTime = pa_wtime() - s->startTime;
               CHK(pa_call_monitor_inner(p, eval[q], rnorm[q], 0, (int)numIts, tau[q]));
            }
         }
      }
      if (have_w && conv > 0) {
         CHK(permute_panel(s, w, ld, blockSize, p0));
         pa_permute_reals(rho_new, 1, blockSize, 1, p0);
      }
      if (have_d && conv > 0) pa_permute_reals(rho_new, 1, blockSize, 1, p0);
      SHRINK();
      if (blockSize <= 0) break;

      if (have_d) {
         /* d already holds K^-1 g + beta d */
         for (i = 0; i < blockSize; i++) {
            const int q = pm[i];
            rho[q] = rho_new[i];
            rho_prev[q] = rho[q]; tau_prev[q] = tau[q]; Theta_prev[q] = Theta[q];
         }
      } else if (numIts + 1 < maxIterations) {
         if (!plain_K) {
            if (have_w) { for (i = 0; i < blockSize; i++) tmp[i] = rho_new[i]; }
            else {
               CHK(apply_projected_preconditioner(s, g, ld, P, blockSize, w, ld));
               CHK(pair_dots_host(s, g, ld, w, ld, blockSize, tmp));
            }
         }
         double beta[64];
         if (ref_ix) for (i = 0; i < blockSize; i++) rho[i] = plain_K ? gg[i] : tmp[i];
         for (i = 0; i < blockSize; i++) {
            const int q = pm[i];
            if (!ref_ix) rho[q] = plain_K ? gg[i] : tmp[i];
            beta[i] = rho[q] / rho_prev[q];
            rho_prev[q] = rho[q]; tau_prev[q] = tau[q]; Theta_prev[q] = Theta[q];
         }
         if (plain_K) {
            CHK(hipk_xpay_cols(s->ctx, RDT(s), RM(s), beta, g, R2(ld), d, R2(ld), blockSize));      /* d = g + beta d */
         } else {
            CHK(hipk_axpy_cols(s->ctx, RDT(s), RM(s), beta, d, R2(ld), w, R2(ld), blockSize));      /* w += beta d */
            char *t = d; d = w; w = t;
         }
      }
   }
#undef SHRINK
   return 0;
}

/* JDQMR correction for the block at V(:, basisSize..), W(:, basisSize..) (x and r), result in x's place.
 * `shifts` are the correction-equation shifts computed by the caller (robust / Ritz / target). */
int pa_correction_jdqmr(pa_solver *s, int basisSize, int blockSize, const double *blockNorms, const int *iev,
      double *shifts, int numLocked, int numConvergedStored, int *touch) {
   primme_params *p = s->p;
   const JD_projectors *jp = &p->correctionParams.projectors;
   char *x = VCOL(s, basisSize), *r = WCOL(s, basisSize), *sol = PCOL(s, s->Jw, s->ld, 4 * blockSize);
   const int sizeEvecs = p->numOrthoConst + (p->locking ? numLocked : numConvergedStored);
   jd_proj P;
   memset(&P, 0, sizeof(P));
   char *Bx = x, *Bq = s->evecs;          /* B x and B evecs: the vectors themselves for a standard problem */
   if (s->B) {
      if (!s->Bevecs) return PRIMME_UNEXPECTED_FAILURE;
      /* the reference reads B x off its B V panel (correction.c:399) and keeps B evecs up to date at every restart; here B comes
       * through the callback: the block's B x now, B evecs for the columns locked since the last call */
      P.Bx = Bx = PCOL(s, s->Jw, s->ld, 6 * p->maxBlockSize);
      P.Bv = PCOL(s, s->Jw, s->ld, 7 * p->maxBlockSize);
      CHK(pa_apply_B(s, x, s->ld, Bx, s->ld, blockSize));
      if (s->ref_soft_alias) Bq = s->evecs;
      else {
         if (s->nBevecs < sizeEvecs) {
            CHK(pa_apply_B(s, ECOL(s, s->nBevecs), s->ldevecs, s->Bevecs + (size_t)s->nBevecs * s->ldevecs * s->es, s->ldevecs, sizeEvecs - s->nBevecs));
            s->nBevecs = sizeEvecs;
         }
         Bq = s->Bevecs;
      }
   }
   if (jp->LeftQ) {
      P.LQ = s->evecs; P.ldLQ = s->ldevecs; P.nLQ = sizeEvecs;
      P.LBQ = Bq; P.ldLBQ = s->ldevecs;
      if (jp->LeftX) {
         if (blockSize <= 1) {   /* keep x next to Q (and B x next to B Q): one projector panel */
            CHK(hipk_copy_cols(s->ctx, s->dt, s->m, x, s->ld, ECOL(s, sizeEvecs), s->ldevecs, blockSize));
            if (s->B) CHK(hipk_copy_cols(s->ctx, s->dt, s->m, Bx, s->ld, Bq + (size_t)sizeEvecs * s->ldevecs * s->es, s->ldevecs, blockSize));
            P.nLQ += blockSize;
         } else { P.LX = x; P.ldLX = s->ld; P.nLX = blockSize; P.LBX = Bx; P.ldLBX = s->ld; }
      }
   } else if (jp->LeftX) { P.LX = x; P.ldLX = s->ld; P.nLX = blockSize; P.LBX = Bx; P.ldLBX = s->ld; }
   P.x = x;
   p->ShiftsForPreconditioner = shifts;
   if (jp->RightQ) {
      P.nRQ = sizeEvecs;
      if (p->correctionParams.precondition && jp->SkewQ) {
         if (!s->evecsHat) return PRIMME_UNEXPECTED_FAILURE;
         P.RQ = s->evecsHat; P.ldRQ = s->ldevecs; P.skewQ = 1;
      } else { P.RQ = Bq; P.ldRQ = s->ldevecs; }
   }
   if (jp->RightX) {
      P.nRX = blockSize;
      if (p->correctionParams.precondition && jp->SkewX) {
         /* K^-1 B x and x'K^-1 B x (reference correction.c:969-977) */
         char *Kx = PCOL(s, s->Jw, s->ld, 5 * p->maxBlockSize);
         CHK(pa_precond(s, Bx, s->ld, Kx, s->ld, blockSize));
         CHK(hipk_pair_dots(s->ctx, s->dt, s->m, x, s->ld, Kx, s->ld, blockSize, s->d_red));
         CHK(pa_reduce(s, s->d_red, SD * blockSize, 0, 0));
         for (int i = 0; i < blockSize; i++) P.xKx[i] = ((const HS *)s->h_red)[i];
         P.RX = Kx; P.ldRX = s->ld; P.skewX = 1;
      } else {
         P.RX = Bx; P.ldRX = s->ld;
         for (int i = 0; i < blockSize; i++) P.xKx[i] = 1.0;
      }
   }

   double evalb[64], rn[64];
   if (blockSize > 64) return PRIMME_FUNCTION_UNAVAILABLE;   /* inner solves with more than 64 right-hand sides */
   for (int i = 0; i < blockSize; i++) { evalb[i] = s->hVals[iev[i]]; rn[i] = blockNorms[i]; }
   p->ShiftsForPreconditioner = shifts;
   const int touch0 = *touch;
   int touch1 = touch0;
   CHK(inner_solve(s, blockSize, x, r, rn, &P, sol, evalb, shifts, &touch1));
   *touch = PA_MAX(*touch, touch1);
   CHK(hipk_copy_cols(s->ctx, s->dt, s->m, sol, s->ld, x, s->ld, blockSize));
   return 0;
}
