/* eigs_common.c — the steps of the host solver that do not depend on the scalar type of the projected problem: the clock,
 * the problem norm, reductions (with the optional all-reduce), the operator / mass matrix / preconditioner wrappers, the
 * default convergence test, the monitor, permutations of real and integer rows and the random number stream.
 *
 * Built once (no eigs_common_z.c): the real and the complex objects of the sources that are compiled twice
 * (eigs_scalar.h) both call these.  Nothing here touches an HS.
 */
#include "eigs_solver.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

double pa_wtime(void) {
   struct timespec ts;
   clock_gettime(CLOCK_MONOTONIC, &ts);
   return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

/* ---- problem norm / machine epsilons (reference auxiliary_eigs.c:498-591) ------ */
double pa_problem_norm(int overrideUser, const primme_params *p) {
   if (p->massMatrixMatvec) {      /* an estimate of |B^-1 A| (auxiliary_eigs.c:567-591) */
      const double user = (p->aNorm > 0.0 && p->invBNorm > 0.0) ? p->aNorm * p->invBNorm : 0.0;
      if (!overrideUser) return user > 0.0 ? user : p->stats.estimateLargestSVal;
      return PA_MAX(user, p->stats.estimateLargestSVal);
   }
   if (!overrideUser) return p->aNorm > 0.0 ? p->aNorm : p->stats.estimateLargestSVal;
   return PA_MAX(p->aNorm > 0.0 ? p->aNorm : 0.0, p->stats.estimateLargestSVal);
}

/* ---- reductions -----------------------------------------------------------------
 * d_buf (device) holds `count` local partial sums.  On return s->h_red[0..count)
 * holds the global sums; if keep_dev, d_buf holds them as well (the next kernel
 * uses them as coefficients).  Restates globalSum_Tprimme (reference
 * auxiliary_eigs.c:391-427) for device-resident partials.
 * When defer_sync is set and no host callback is involved, the device->host copy
 * is only enqueued; the caller must hipk_sync before reading h_red. */
int pa_reduce(pa_solver *s, double *d_buf, int count, int keep_dev, int defer_sync) {
   primme_params *p = s->p;
   if (count <= 0) return 0;
   /* d_buf lies in [d_red, d_red + 2*red_cap): the second half holds the fused kernel's overlaps */
   if (d_buf < s->d_red || (size_t)(d_buf - s->d_red) + (size_t)count > 3 * (size_t)s->red_cap + 64) return PRIMME_UNEXPECTED_FAILURE;
   const int parallel = s->parallel;
   double t0 = parallel ? pa_wtime() : 0.0;
   if (parallel && s->dev_comm) {
      if (hipk_xreduce_covered(s->ctx, d_buf, count)) {
         /* the producing launch's second stage exchanged its sums with the other ranks itself (peer-to-peer
          * transport, hipk_xreduce_arm): d_buf and the pinned mirror already hold the global sums */
         if (!defer_sync) CHK(hipk_wait_results(s->ctx));
      } else {
      /* peer-to-peer transport: reduction, mirror and completion flag are one launch */
      int rcp = pa_comm_allreduce_publish(p->commInfo, s->ctx, d_buf, count);
      if (rcp < 0) return PRIMME_PARALLEL_FAILURE;
      if (rcp == 0) {
         if (!defer_sync) CHK(hipk_wait_results(s->ctx));
      } else {
      CHK(pa_comm_allreduce_device(p->commInfo, d_buf, count, hipk_ctx_stream(s->ctx)));
      /* the global sums reach the pinned mirror through a one-block launch that also publishes the completion flag
       * (the wait is then a spin on pinned memory, as on one rank); fallback: copy + stream synchronisation */
      static int no_publish = -1;      /* PRIMME_AMD_NO_PUBLISH=1: measurement knob, read once */
      if (no_publish < 0) no_publish = getenv("PRIMME_AMD_NO_PUBLISH") != NULL;
      rcp = no_publish ? 1 : hipk_publish_results(s->ctx, d_buf, count);
      if (rcp < 0) return PRIMME_UNEXPECTED_FAILURE;
      if (rcp == 0) {
         if (!defer_sync) CHK(hipk_wait_results(s->ctx));
      } else {
         CHK(hipk_d2h(s->ctx, s->h_red + (d_buf - s->d_red), d_buf, (size_t)count * sizeof(double)));
         if (!defer_sync) CHK(hipk_sync(s->ctx));
      }
      }
      }
      if (!defer_sync && pa_comm_failed(p->commInfo)) return PRIMME_PARALLEL_FAILURE;
   } else {
      /* the reduction kernels already stored the local sums in h_red (zero-copy mirror) */
      if (parallel) {
         CHK(hipk_sync(s->ctx));
         double *hb = s->h_red + (d_buf - s->d_red);
         CHK(pa_call_global_sum(p, hb, count));
         if (keep_dev) CHK(hipk_h2d(s->ctx, d_buf, hb, (size_t)count * sizeof(double)));
      } else if (!defer_sync) {
         /* the reduction whose result is wanted was the last launch: wait for its completion flag */
         CHK(hipk_wait_results(s->ctx));
      }
   }
   if (parallel) {
      p->stats.numGlobalSum++;
      p->stats.volumeGlobalSum += count;
      p->stats.timeGlobalSum += pa_wtime() - t0;
   }
   return 0;
}

/* G = W(:,0:k)' Q for the locked / constraint vectors Q (projection column from W'r,
 * eigs_conv.c): one TN panel product after a restart. */
int pa_refresh_wtq(pa_solver *s, int basisSize, int nLk) {
   if (s->fov_carry && s->wtq_rows == basisSize && s->wtq_L == nLk) return 0;   /* the restart transformed it */
   s->wtq_rows = -1; s->wtq_L = nLk;
   if (!s->wtr_enabled || !s->wtq || basisSize > HIPK_WTR_MAX_K || nLk > HIPK_WTR_MAX_K) return 0;
   if (nLk > 0 && basisSize > 0) {
      if (basisSize * nLk > s->red_cap) return 0;
      hipk_seg seg = {s->W, s->ld, basisSize};
      CHK(hipk_panel_dots(s->ctx, s->dt, s->m, &seg, 1, s->evecs, s->ldevecs, nLk, s->d_red, basisSize));
      CHK(pa_reduce(s, s->d_red, basisSize * nLk, 0, 0));
      for (int l = 0; l < nLk; l++)
         for (int j = 0; j < basisSize; j++) s->wtq[j + (size_t)l * s->K] = s->h_red[j + (size_t)l * basisSize];
   }
   s->wtq_rows = basisSize;
   return 0;
}

int pa_trace_errors(void) {
   static int on = -1;
   if (on < 0) on = getenv("PRIMME_AMD_TRACE_ERRORS") != NULL;
   return on;
}

/* global sum of a few host scalars (cost-model ratios): through the same path as the
 * device partials so that every communicator flavour is covered */
int pa_reduce_host(pa_solver *s, double *buf, int count) {
   if (count <= 0 || !s->parallel) return 0;
   CHK(hipk_sync(s->ctx));
   memcpy(s->h_red, buf, (size_t)count * sizeof(double));
   if (s->dev_comm) CHK(hipk_h2d(s->ctx, s->d_red, s->h_red, (size_t)count * sizeof(double)));
   CHK(pa_reduce(s, s->d_red, count, 0, 0));
   memcpy(buf, s->h_red, (size_t)count * sizeof(double));
   return 0;
}

/* ---- W(:,c0:c0+nc) = A * V(:,c0:c0+nc)  (reference auxiliary_eigs.c:183-230) ---- */
int pa_matvec(pa_solver *s, char *Vp, int64_t ldV, char *Wp, int64_t ldW, int c0, int nc) {
   primme_params *p = s->p;
   if (nc <= 0) return 0;
   double t0 = pa_wtime();
   int ierr = 0;
   PRIMME_INT ldx = ldV, ldy = ldW;
   p->matrixMatvec(PCOL(s, Vp, ldV, c0), &ldx, PCOL(s, Wp, ldW, c0), &ldy, &nc, p, &ierr);
   if (ierr) return PRIMME_USER_FAILURE;
   if (s->phase_timing) CHK(hipk_sync(s->ctx));
   p->stats.timeMatvec += pa_wtime() - t0;
   p->stats.numMatvecs += nc;
   return 0;
}

/* ---- Y(:,0:nc) = B * X(:,0:nc)  (reference massMatrixMatvec_Sprimme, auxiliary_eigs.c:250-290) ---- */
int pa_apply_B(pa_solver *s, char *X, int64_t ldX, char *Y, int64_t ldY, int nc) {
   primme_params *p = s->p;
   if (nc <= 0) return 0;
   double t0 = pa_wtime();
   /* in blocks of the width the callback was promised (maxBlockSize; the initial basis hands over more at once, init.c:210) */
   int ierr = 0;
   PRIMME_INT ldx = ldX, ldy = ldY;
   p->massMatrixMatvec(X, &ldx, Y, &ldy, &nc, p, &ierr);
   if (ierr) return PRIMME_USER_FAILURE;
   if (s->phase_timing) CHK(hipk_sync(s->ctx));
   p->stats.timeMatvec += pa_wtime() - t0;
   p->stats.numMatvecs += nc;      /* the reference counts applications of B with those of A (auxiliary_eigs.c:283) */
   return 0;
}

/* ---- y = K^-1 x or copy (reference auxiliary_eigs.c:317-364) -------------------- */
int pa_precond(pa_solver *s, char *X, int64_t ldX, char *Y, int64_t ldY, int nc) {
   primme_params *p = s->p;
   if (nc <= 0) return 0;
   double t0 = pa_wtime();
   if (p->correctionParams.precondition) {
      int ierr = 0;
      PRIMME_INT ldx = ldX, ldy = ldY;
      p->applyPreconditioner(X, &ldx, Y, &ldy, &nc, p, &ierr);
      if (ierr) return PRIMME_USER_FAILURE;
      p->stats.numPreconds += nc;
   } else {
      CHK(hipk_copy_cols(s->ctx, s->dt, s->m, X, ldX, Y, ldY, nc));
   }
   if (s->phase_timing) CHK(hipk_sync(s->ctx));
   p->stats.timePrecond += pa_wtime() - t0;
   return 0;
}

/* default convTestFun (reference src/eigs/primme_c.c:555-570) */
void pa_conv_test_absolute(double *eval, void *evec, double *rNorm, int *isConv,
      primme_params *p, int *ierr) {
   (void)eval; (void)evec;
   /* machine epsilon of the working precision is kept in convtest when we install it */
   double meps = p->convtest ? *(double *)p->convtest : PA_EPS;
   *isConv = *rNorm < PA_MAX(p->eps, meps * (p->massMatrixMatvec ? 1 : 2)) * pa_problem_norm(0, p);
   *ierr = 0;
}

/* primme->monitorFun, or the reference's default report when none is installed */
void pa_monitor(pa_solver *s, double *basisEvals, int basisSize, int *basisFlags, int *iblock,
      int blockSize, double *basisNorms, int numConverged, double *lockedEvals, int numLocked,
      int *lockedFlags, double *lockedNorms, primme_event event) {
   primme_params *p = s->p;
   p->stats.elapsedTime = pa_wtime() - s->startTime;
   if (!p->monitorFun) {
      /* the reference's default report (primme_c.c:602-700), same lines so that logs stay comparable */
      if (!p->outputFile || p->procID != 0 || p->printLevel < 2) return;
      const int found = p->locking ? numLocked : numConverged;
      if (event == primme_event_outer_iteration && p->printLevel >= 3) {
         for (int i = 0; i < blockSize; i++)
            fprintf(p->outputFile, "OUT %lld conv %d blk %d MV %lld Sec %E EV %13E |r| %.3E\n",
                  (long long)p->stats.numOuterIterations, found, i, (long long)p->stats.numMatvecs, p->stats.elapsedTime,
                  basisEvals[iblock[i]], basisNorms[iblock[i]]);
      } else if (event == primme_event_converged && ((!p->locking && p->printLevel >= 2) || (p->locking && p->printLevel >= 5))) {
         fprintf(p->outputFile, "#Converged %d eval[ %d ]= %13E norm %e Mvecs %lld Time %g\n", numConverged, iblock[0],
               basisEvals[iblock[0]], basisNorms[iblock[0]], (long long)p->stats.numMatvecs, p->stats.elapsedTime);
      } else if (event == primme_event_locked) {
         fprintf(p->outputFile, "Lock epair[ %d ]= %13E norm %.4e Mvecs %lld Time %.4e Flag %d\n", numLocked,
               lockedEvals[numLocked - 1], lockedNorms[numLocked - 1], (long long)p->stats.numMatvecs, p->stats.elapsedTime,
               lockedFlags[numLocked - 1]);
      }
      return;
   }
   (void)pa_call_monitor(p, basisEvals, basisSize, basisFlags, iblock, blockSize, basisNorms, numConverged,
         lockedEvals, numLocked, lockedFlags, lockedNorms, event);
}

/* diagnostics of the last solve of this process: iterations enqueued ahead of the host / adopted (include/primme_amd.h) */
long pa_last_pre[2];
void primme_amd_prelaunch_stats(long *launched, long *adopted) {
   if (launched) *launched = pa_last_pre[0];
   if (adopted) *adopted = pa_last_pre[1];
}

/* diagnostics of this process (include/primme_amd.h): inner QMR steps of the real solver taken / taken with one host
 * synchronisation since the last call (counted in eigs_jd.c) */
long pa_qmr_steps[2];
void primme_amd_qmr_step_stats(long *steps, long *one_synchronisation) {
   if (steps) *steps = pa_qmr_steps[0];
   if (one_synchronisation) *one_synchronisation = pa_qmr_steps[1];
   pa_qmr_steps[0] = pa_qmr_steps[1] = 0;
}

/* type-independent permutations: new entry i = old entry perm[i] */
void pa_permute_reals(double *A, int mrows, int n, int lda, const int *perm) { pa_permute_cols(A, mrows, n, lda, perm); }
void pa_permute_ints(int *a, int n, const int *perm) {
   if (n <= 0) return;
   int *tmp = (int *)malloc((size_t)n * sizeof(int));
   for (int j = 0; j < n; j++) tmp[j] = a[perm[j]];
   memcpy(a, tmp, (size_t)n * sizeof(int));
   free(tmp);
}

/* LAPACK xLARNV(idist = 2) stream, restated: 48-bit multiplicative congruential
 * generator x <- a*x mod 2^48, a = 33952834046453, uniform(-1,1) = 2*x/2^48 - 1.
 * iseed holds the state as four base-4096 digits (updated on exit).  Verified
 * bit-for-bit against the LAPACK in this image (tests/test_dense_host.py).
 * The reference calls this through Num_larnv_Sprimme (blaslapack.c:938-988). */
void pa_larnv_uniform11(int64_t iseed[4], int64_t n, double *x) {
   const uint64_t A = 33952834046453ULL, MASK = (1ULL << 48) - 1;
   uint64_t s = ((((uint64_t)iseed[0] * 4096 + (uint64_t)iseed[1]) * 4096 + (uint64_t)iseed[2]) * 4096 +
                 (uint64_t)iseed[3]) & MASK;
   for (int64_t i = 0; i < n; i++) {
      s = (s * A) & MASK;
      x[i] = 2.0 * ((double)s / 281474976710656.0) - 1.0;
   }
   iseed[0] = (int64_t)((s >> 36) & 4095);
   iseed[1] = (int64_t)((s >> 24) & 4095);
   iseed[2] = (int64_t)((s >> 12) & 4095);
   iseed[3] = (int64_t)(s & 4095);
}
