/* eigs_internal.h — declarations shared by the host side of the solver: every function that more than one file
 * uses and that takes no pa_solver (those are in eigs_solver.h), grouped by the file that defines it.  The definer
 * and every caller include this header, the .hip files that define the last group as well as the C sources, so a
 * prototype exists once and the build (-Werror=missing-prototypes) holds each definition against it. */
#ifndef EIGS_INTERNAL_H
#define EIGS_INTERNAL_H

#include <stdint.h>
#include "primme_amd.h"
#include "primme_amd_kernels.h"
#include "eigs_scalar.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PA_MIN(a, b) ((a) < (b) ? (a) : (b))
#define PA_MAX(a, b) ((a) > (b) ? (a) : (b))
#define PA_EPS 2.220446049250313e-16 /* double */

struct primme_svds_params;

/* ---- eigs_dense.c: dense helpers; HS = double, or double complex in the complex objects (Hermitian / unitary
 * variants: ' reads as conjugate transpose) */
int  pa_sym_eig(int n, const HS *A, int lda, double *evals, HS *Z, int ldz);
int  pa_sym_eig_gen(int n, const HS *H, int ldh, const HS *G, int ldg, double *evals,
      HS *Z, int ldz);
int  pa_potrf_upper(int n, HS *A, int lda);
void pa_trsm_left_upper_trans(int n, int nb, const HS *U, int ldu, HS *B, int ldb);
void pa_trsm_left_upper(int n, int nb, const HS *U, int ldu, HS *B, int ldb);
void pa_trsm_right_upper(int mb, int n, const HS *U, int ldu, HS *B, int ldb);
void pa_permute_cols(HS *A, int mrows, int n, int lda, const int *perm);
void pa_submatrix(const HS *X, int nx, int ldx, const HS *H, int nh, int ldh, HS *R,
      int ldr);
/* A = U diag(S) V' of a small square matrix, S descending */
int  pa_svd(const HS *A, int ldA, int n, HS *U, int ldU, double *S, HS *V, int ldV);

/* ---- eigs_common.c: what is the same for both scalar types and exists once */
/* |A| (|B^-1 A| with a mass matrix) from the user's norms and the running estimates */
double pa_problem_norm(int overrideUser, const primme_params *p);
/* default convTestFun */
void pa_conv_test_absolute(double *eval, void *evec, double *rNorm, int *isConv, primme_params *p, int *ierr);
void pa_permute_reals(double *A, int mrows, int n, int lda, const int *perm);   /* Ritz values and other real rows */
void pa_permute_ints(int *a, int n, const int *perm);
/* LAPACK xLARNV(idist = 2) stream */
void pa_larnv_uniform11(int64_t iseed[4], int64_t n, double *x);
extern long pa_last_pre[2];   /* pre-enqueued iterations of the last solve (launched, adopted) */
extern long pa_qmr_steps[2];  /* inner QMR steps of the real solver since the last query (all, one-synchronisation ones) */

/* ---- eigs_block.c */
/* fG(:, n0:n) <- Cholesky update given the new columns G(:, n0:n) */
int pa_update_cholesky(const HS *G, int ldG, HS *fG, int ldfG, int n0, int n);

/* ---- eigs_ops.c */
/* orthonormalise the coefficient vector x against the columns of Q in the G inner product (host) */
int pa_ortho_local_vec(HS *x, int n, const HS *Q, int ldQ, int nQ, const HS *G,
      int ldG, double *R, int64_t iseed[4]);

/* ---- eigs_conv.c */
/* p[i] = column of Vp (m x nV) closest in angle to column i of Wn (m x n), i in [n0,n) */
void pa_map_vecs(const HS *Vp, int mrows, int nV, int ldV, const HS *Wn, int n0, int n,
      int ldW, int *pm);

/* ---- eigs_main.c: internal entry for the svds front end (eigenvalues and residual norms always in double); the
 * front ends that exist once reach the complex instantiation (eigs_main_z.c and friends) by its own name */
int pa_eigs_solve(void *evals_out, void *evecs, void *resNorms_out, primme_params *p, hipk_dtype dt, int out_double);
#ifndef PA_COMPLEX   /* (in the complex objects the line above already reads pa_eigs_solve_z: a second one would be redundant) */
int pa_eigs_solve_z(void *evals_out, void *evecs, void *resNorms_out, primme_params *p, hipk_dtype dt, int out_double);
#endif

/* ---- eigs_callbacks.c: user callbacks called with the operand type they declare */
int pa_call_global_sum(primme_params *p, double *buf, int count);
int pa_call_conv_test(primme_params *p, double eval, void *evec, double rnorm, int *isconv);
int pa_call_monitor(primme_params *p, double *basisEvals, int basisSize, int *basisFlags, int *iblock, int blockSize,
      double *basisNorms, int numConverged, double *lockedEvals, int numLocked, int *lockedFlags, double *lockedNorms,
      primme_event event);
int pa_call_monitor_inner(primme_params *p, double eval, double resNorm, int counts, int innerIts, double lsRes);
int pa_svds_call_global_sum(struct primme_svds_params *ps, double *buf, int count);
int pa_svds_call_conv_test(struct primme_svds_params *ps, double sval, void *leftsvec, void *rightsvec, double rnorm,
      int *method, int *isconv);

/* ---- eigs_complex.c: complex-independence sweep shared by hip_zprimme and hip_zprimme_svds */
typedef int (*pa_sum_fn)(void *who, double *buf, int count);
int pa_complex_sweep(hipk_ctx *ctx, hipk_dtype dtr, int64_t mr, int64_t ldr, char *cand, int ncand, char *Z, char *rot,
      int nwant, double *d_s, double *h_s, pa_sum_fn sum, void *who, int *picked, int *nacc);

/* ---- eigs_params.c: parameter handling */
int pa_check_input(const void *evals, const void *evecs, const void *resNorms,
      const primme_params *primme, double machine_eps);

/* ---- svds_main.c */
/* the library's own operator can run the one-launch tail (scale + A t + t'At) of the normal equations on one rank */
int pa_svds_can_fuse(const primme_params *primme);
/* xout = a t, y = A'A xout (or A A' xout), dot_dev[0] = xout'y: everything enqueued, nothing waited for */
int pa_svds_apply_scaled(primme_params *primme, hipk_ctx *ctx, const void *t, const double *norm2_dev, void *xout, void *y,
      double *dot_dev);
/* the installed convergence test is the default one on a triplet, which does not look at the vectors */
int pa_svds_conv_test_is_vector_free(const primme_params *p);
/* the native complex front end (called by svds_complex.c's hip_zprimme_svds / hip_cprimme_svds) */
int pa_svds_solve_native_complex(void *svals, void *svecs, void *resNorms, struct primme_svds_params *ps, int single);

/* ---- defined on the device side (comm_rccl.hip, hipk_core.hip, amd_operator.hip), called from C; the plain-C
 * stand-ins of the host-only test build define the same names against this text */
/* communicator (comm_rccl.hip): device all-reduce used when primme->globalSumReal ==
 * primme_amd_global_sum */
int pa_comm_allreduce_device(void *commInfo, double *dbuf, int count, void *hip_stream);
/* peer-to-peer transport (comm_ipc.hip): reduction + pinned mirror + completion flag in one launch; 1 = not on this transport */
int pa_comm_allreduce_publish(void *commInfo, hipk_ctx *ctx, double *dbuf, int count);
/* let the context's second-stage launches reduce across the ranks themselves (no-op on RCCL); 0 = attached */
int pa_comm_attach_ctx(void *commInfo, hipk_ctx *ctx);
/* non-zero after a device-side wait of the transport ran into its time limit (a rank left the collective sequence) */
int pa_comm_failed(void *commInfo);
/* arm the NEXT second-stage launch on the context as a cross-rank one (only with an attached communicator) */
void hipk_xreduce_arm(hipk_ctx *ctx);
/* 1 when a communicator of the peer-to-peer transport is attached to the context (arming has an effect) */
int hipk_xreduce_available(hipk_ctx *ctx);
/* 1 when [buf, buf+count) was produced by an armed launch since the last call: the sums are already global and
 * published (the record is consumed) */
int hipk_xreduce_covered(hipk_ctx *ctx, const double *buf, int count);
/* 1 when the singular value operator holds the whole matrix (no communicator) */
int primme_amd_svds_operator_is_local(const void *op);

#ifdef __cplusplus
}
#endif

#endif
