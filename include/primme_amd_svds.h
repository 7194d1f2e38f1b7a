/* primme_amd_svds.h — boundary B1 for singular value problems.
 *
 * Same types, field order and calling conventions as the reference's
 * include/primme_svds.h:46-168 (sizeof(primme_svds_params) = 1720 on x86-64), so a program
 * written against dprimme_svds() / cublas_dprimme_svds() switches by renaming the solver call:
 *
 *     reference                                   this library
 *     primme_svds_initialize  (interface.c:108)   primme_svds_initialize
 *     primme_svds_set_method  (interface.c:218)   primme_svds_set_method
 *     cublas_dprimme_svds     (primme_svds.h:264) hip_dprimme_svds   (svecs = DEVICE pointer)
 *     cublas_sprimme_svds     (primme_svds.h:260) hip_sprimme_svds
 *
 * Covered on the device path: the normal-equations method (A'A when n <= m, AA' otherwise;
 * reference primme_svds_interface.c:231-235), the augmented operator [0 A'; A 0] and the hybrid
 * default, for the largest / smallest / closest_abs singular triplets.  What the eigensolver does
 * not cover (the refined extraction with explicit_I, i.e. interior targets with block size > 1 or
 * in single precision) comes back as PRIMME_FUNCTION_UNAVAILABLE - 100 / - 200, never a CPU
 * fallback.
 */
#ifndef PRIMME_AMD_SVDS_H
#define PRIMME_AMD_SVDS_H

#include "primme_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { primme_svds_largest, primme_svds_smallest, primme_svds_closest_abs } primme_svds_target;
typedef enum {
   primme_svds_default, primme_svds_hybrid, primme_svds_normalequations, primme_svds_augmented
} primme_svds_preset_method;
typedef enum {
   primme_svds_op_none, primme_svds_op_AtA, primme_svds_op_AAt, primme_svds_op_augmented
} primme_svds_operator;

typedef struct primme_svds_stats {
   PRIMME_INT numOuterIterations, numRestarts, numMatvecs, numPreconds;
   PRIMME_INT numGlobalSum, numBroadcast, volumeGlobalSum, volumeBroadcast;
   double numOrthoInnerProds, elapsedTime, timeMatvec, timePrecond, timeOrtho;
   double timeGlobalSum, timeBroadcast;
   PRIMME_INT lockingIssue;
} primme_svds_stats;

struct primme_svds_params;
typedef void (*primme_svds_block_op)(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy,
      int *blockSize, int *transpose, struct primme_svds_params *primme_svds, int *ierr);

typedef struct primme_svds_params {
   primme_params primme;        /* first-stage eigenproblem (must stay the first field) */
   primme_params primmeStage2;  /* hybrid second stage */
   PRIMME_INT m, n;             /* rows, columns of A */
   primme_svds_block_op matrixMatvec;        primme_op_datatype matrixMatvec_type;
   primme_svds_block_op applyPreconditioner; primme_op_datatype applyPreconditioner_type;
   int numProcs, procID;
   PRIMME_INT mLocal, nLocal;
   void *commInfo;
   void (*globalSumReal)(void *sendBuf, void *recvBuf, int *count,
         struct primme_svds_params *primme_svds, int *ierr);
   primme_op_datatype globalSumReal_type;
   void (*broadcastReal)(void *buffer, int *count, struct primme_svds_params *primme_svds, int *ierr);
   primme_op_datatype broadcastReal_type;
   int numSvals;
   primme_svds_target target;
   int numTargetShifts;
   double *targetShifts;
   primme_svds_operator method, methodStage2;
   void *matrix, *preconditioner;
   int locking, numOrthoConst;
   double aNorm, eps;
   int precondition, initSize, maxBasisSize, maxBlockSize;
   PRIMME_INT maxMatvecs;
   PRIMME_INT iseed[4];
   int printLevel;
   primme_op_datatype internalPrecision;
   FILE *outputFile;
   struct primme_svds_stats stats;
   void (*convTestFun)(double *sval, void *leftsvec, void *rightsvec, double *rNorm, int *method,
         int *isconv, struct primme_svds_params *primme_svds, int *ierr);
   primme_op_datatype convTestFun_type;
   void *convtest;
   void (*monitorFun)(void *basisSvals, int *basisSize, int *basisFlags, int *iblock, int *blockSize,
         void *basisNorms, int *numConverged, void *lockedSvals, int *numLocked, int *lockedFlags,
         void *lockedNorms, int *inner_its, void *LSRes, const char *msg, double *time,
         primme_event *event, int *stage, struct primme_svds_params *primme_svds, int *err);
   primme_op_datatype monitorFun_type;
   void *monitor;
   void *queue;            /* hipStream_t* of the caller, or NULL */
   const char *profile;
} primme_svds_params;

/* labels of the members (reference include/primme_svds.h:166-230); the numeric values are ABI */
typedef enum {
   PRIMME_SVDS_invalid_label = 0,
   PRIMME_SVDS_primme = 1, PRIMME_SVDS_primmeStage2 = 2, PRIMME_SVDS_m = 3, PRIMME_SVDS_n = 4, PRIMME_SVDS_matrixMatvec = 5,
   PRIMME_SVDS_matrixMatvec_type = 6, PRIMME_SVDS_applyPreconditioner = 7, PRIMME_SVDS_applyPreconditioner_type = 8,
   PRIMME_SVDS_numProcs = 9, PRIMME_SVDS_procID = 10, PRIMME_SVDS_mLocal = 11, PRIMME_SVDS_nLocal = 12,
   PRIMME_SVDS_commInfo = 13, PRIMME_SVDS_globalSumReal = 14, PRIMME_SVDS_globalSumReal_type = 15,
   PRIMME_SVDS_broadcastReal = 16, PRIMME_SVDS_broadcastReal_type = 17, PRIMME_SVDS_numSvals = 18, PRIMME_SVDS_target = 19,
   PRIMME_SVDS_numTargetShifts = 20, PRIMME_SVDS_targetShifts = 21, PRIMME_SVDS_method = 22, PRIMME_SVDS_methodStage2 = 23,
   PRIMME_SVDS_matrix = 24, PRIMME_SVDS_preconditioner = 25, PRIMME_SVDS_locking = 26, PRIMME_SVDS_numOrthoConst = 27,
   PRIMME_SVDS_aNorm = 28, PRIMME_SVDS_eps = 29, PRIMME_SVDS_precondition = 30, PRIMME_SVDS_initSize = 31,
   PRIMME_SVDS_maxBasisSize = 32, PRIMME_SVDS_maxBlockSize = 33, PRIMME_SVDS_maxMatvecs = 34, PRIMME_SVDS_iseed = 35,
   PRIMME_SVDS_printLevel = 36, PRIMME_SVDS_internalPrecision = 37, PRIMME_SVDS_outputFile = 38,
   PRIMME_SVDS_stats_numOuterIterations = 39, PRIMME_SVDS_stats_numRestarts = 40, PRIMME_SVDS_stats_numMatvecs = 41,
   PRIMME_SVDS_stats_numPreconds = 42, PRIMME_SVDS_stats_numGlobalSum = 43, PRIMME_SVDS_stats_volumeGlobalSum = 44,
   PRIMME_SVDS_stats_numBroadcast = 45, PRIMME_SVDS_stats_volumeBroadcast = 46, PRIMME_SVDS_stats_numOrthoInnerProds = 47,
   PRIMME_SVDS_stats_elapsedTime = 48, PRIMME_SVDS_stats_timeMatvec = 49, PRIMME_SVDS_stats_timePrecond = 50,
   PRIMME_SVDS_stats_timeOrtho = 51, PRIMME_SVDS_stats_timeGlobalSum = 52, PRIMME_SVDS_stats_timeBroadcast = 53,
   PRIMME_SVDS_stats_lockingIssue = 54, PRIMME_SVDS_convTestFun = 55, PRIMME_SVDS_convTestFun_type = 56,
   PRIMME_SVDS_convtest = 57, PRIMME_SVDS_monitorFun = 58, PRIMME_SVDS_monitorFun_type = 59, PRIMME_SVDS_monitor = 60,
   PRIMME_SVDS_queue = 61, PRIMME_SVDS_profile = 62
} primme_svds_params_label;

primme_svds_params *primme_svds_params_create(void);
int primme_svds_params_destroy(primme_svds_params *primme_svds);
void primme_svds_initialize(primme_svds_params *primme_svds);
int primme_svds_set_method(primme_svds_preset_method method, primme_preset_method methodStage1,
      primme_preset_method methodStage2, primme_svds_params *primme_svds);
void primme_svds_set_defaults(primme_svds_params *primme_svds);
void primme_svds_free(primme_svds_params *primme_svds);

/* Prints the configuration to primme_svds.outputFile in the reference's format (src/svds/primme_svds_interface.c:421): the
 * block itself, then primme_svds.primme under the prefix "primme" when method is set and primme_svds.primmeStage2 under
 * "primmeStage2" when methodStage2 is. */
void primme_svds_display_params(primme_svds_params primme_svds);
/* The member interface of primme_amd.h for primme_svds_params, with the same conventions for `value`.  The labels primme and
 * primmeStage2 are pointers that can be read (the address of the nested block, to be used with primme_get_member /
 * primme_set_member) and not set; stats_numGlobalSum, stats_numBroadcast and stats_lockingIssue cannot be set either.
 * iseed is reported with arity 1 although get and set move four values.  primme_svds_constant_info also knows every name of
 * primme_constant_info; in primme_svds_enum_member_info the preset methods answer to PRIMME_SVDS_commInfo. */
int primme_svds_get_member(primme_svds_params *primme_svds, primme_svds_params_label label, void *value);
int primme_svds_set_member(primme_svds_params *primme_svds, primme_svds_params_label label, void *value);
int primme_svds_member_info(primme_svds_params_label *label, const char **label_name, primme_type *type, int *arity);
int primme_svds_constant_info(const char *label_name, int *value);
int primme_svds_enum_member_info(primme_svds_params_label label, int *value, const char **value_name);

/* svecs: DEVICE array [U (mLocal x numSvals, ld mLocal) | V (nLocal x numSvals, ld nLocal)] behind
 * numOrthoConst constraint columns of each; svals, resNorms: host arrays.  The user matvec gets
 * device pointers and runs on the stream in *primme_svds->queue (set by the solver when NULL). */
int hip_dprimme_svds(double *svals, double *svecs, double *resNorms, primme_svds_params *primme_svds);
int hip_sprimme_svds(float *svals, float *svecs, float *resNorms, primme_svds_params *primme_svds);
/* complex matrices (reference primme_svds.h:242-243, :268-271: cublas_zprimme_svds / cublas_cprimme_svds): svecs holds
 * complex vectors (re, im interleaved); through the real-equivalent form, csrc/svds_complex.c */
int hip_zprimme_svds(double *svals, void *svecs, double *resNorms, primme_svds_params *primme_svds);
int hip_cprimme_svds(float *svals, void *svecs, float *resNorms, primme_svds_params *primme_svds);

/* The reference's CPU entry points with their HOST-pointer contract (reference include/primme_svds.h:236-243,
 * src/svds/primme_svds_c.c:113-118; BASELINE configs[4] is worded with dprimme_svds): svecs is a host array
 * [Uc U | Vc V], the callbacks get host pointers, primme_svds->queue must be NULL.  A program written against the
 * CPU library (examples/ex_svds_dseq.c) relinks unchanged; the solve runs on the device and every operator
 * application is staged through pinned host memory (csrc/svds_hostapi.c) — the plumbing path; hand
 * hip_?primme_svds a device callback or the library's CSR operator for the device rate. */
int dprimme_svds(double *svals, double *svecs, double *resNorms, primme_svds_params *primme_svds);
int sprimme_svds(float *svals, float *svecs, float *resNorms, primme_svds_params *primme_svds);
int zprimme_svds(double *svals, void *svecs, double *resNorms, primme_svds_params *primme_svds);
int cprimme_svds(float *svals, void *svecs, float *resNorms, primme_svds_params *primme_svds);

/* ---- ready-made matvec for a device-resident CSR matrix and its transpose ----------------
 * primme_svds->matrix = handle from primme_amd_svds_operator_create (A and A' are both kept in
 * CSR: the transposed product is then the same coalesced row-tile kernel instead of a scatter
 * with atomics).  Replaces the hand-written callbacks of the reference's examples
 * (examples/ex_svds_dseq.c) and of tests/COMMON/mat.c (CSRMatrixMatvecSVD). */
typedef struct primme_amd_svds_operator primme_amd_svds_operator;
struct hipk_ctx;
int primme_amd_svds_operator_create(primme_amd_svds_operator **op, struct hipk_ctx *ctx, int dt,
      int64_t m, int64_t n, const int32_t *rowptr_host, const int32_t *colind_host,
      const void *values_host);
/* Row-partitioned A across the ranks of a communicator (BASELINE configs[4]: 8 M x 2 M over 8
 * GPUs): this rank owns rows [row0, row0+mLocal) of A and entries [col0, col0+nLocal) of every
 * n-vector, nLocal equal on all ranks.  rowptr/colind (GLOBAL column numbers)/values describe the
 * local rows.  y = A x: all-gather of x, local product.  y = A' x: local product with the local
 * rows' transpose into a full n-vector, reduce-scatter.  comm = primme_amd_comm* (primme_amd_comm.h). */
int primme_amd_svds_operator_create_dist(primme_amd_svds_operator **op, struct hipk_ctx *ctx, int dt,
      int64_t mLocal, int64_t n, int64_t nLocal, const int32_t *rowptr_host, const int32_t *colind_host,
      const void *values_host, void *comm);
int primme_amd_svds_operator_destroy(primme_amd_svds_operator *op);
/* on = 1: the matrix is the real-equivalent form (2m x 2n, primme_amd_csr_complex_to_real) of a complex one and
 * primme_amd_svds_matvec is called by hip_zprimme_svds / hip_cprimme_svds with leading dimensions counted in
 * complex elements (single rank) */
int primme_amd_svds_operator_set_complex(primme_amd_svds_operator *op, int on);
/* globalSumReal with the primme_svds signature over the same communicator
 * (primme_svds->commInfo = primme_amd_comm*).  When hip_dprimme_svds sees this function installed
 * it gives the eigensolver the in-stream RCCL reduction of primme_amd_global_sum. */
void primme_amd_svds_global_sum(void *sendBuf, void *recvBuf, int *count,
      struct primme_svds_params *primme_svds, int *ierr);
void primme_amd_svds_matvec(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy, int *blockSize,
      int *transpose, struct primme_svds_params *primme_svds, int *ierr);
/* Ready-made applyPreconditioner: the diagonal preconditioner of the reference's test driver for
 * singular value problems (tests/COMMON/mat.c:353-426, driver.PrecChoice = jacobi): y = x ./
 * (diag(A'A) - shift^2) for the A'A operator, x ./ (diag(AA') - shift^2) for AA', both halves for the
 * augmented operator.  set_jacobi builds the two diagonals from the host CSR arrays the operator
 * was created from (single-rank operators); primme_svds->preconditioner = the operator handle. */
int primme_amd_svds_operator_set_jacobi(primme_amd_svds_operator *op, const int32_t *rowptr_host,
      const int32_t *colind_host, const void *values_host, double shift);
void primme_amd_svds_jacobi_precond(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy, int *blockSize,
      int *mode, struct primme_svds_params *primme_svds, int *ierr);
/* Ready-made applyPreconditioner: the Chebyshev polynomial preconditioner of primme_amd.h for singular value problems.
 * The arguments of set_chebyshev are in SINGULAR VALUE units: [slo, shi] is the part of the singular spectrum to damp, sshift
 * the target outside (slo, shi) (an end of the interval is allowed).  With lo = slo^2, hi = shi^2, sigma = sshift^2 let p be
 * the polynomial of primme_amd_chebyshev_precond: the steps-th Chebyshev iterate for (M - sigma I) y = x from y = 0.  Then
 *    mode primme_svds_op_AtA        (n-vectors)            y = p(A'A) x
 *    mode primme_svds_op_AAt        (m-vectors)            y = p(AA') x
 *    mode primme_svds_op_augmented  ([v; u], n then m)     y = (B + sshift I) diag(p(A'A), p(AA')) x,  B = [0 A'; A 0]
 *    any other mode                                        *ierr = 1
 * On an eigenvector of B with eigenvalue l the augmented result is (1 - q(l^2)) / (l - sshift), q the residual polynomial: an
 * approximation of (B - sshift I)^-1 that is symmetric and commutes with B, for the smallest, largest and interior targets.
 * set_chebyshev returns -1 for steps < 1, slo < 0 or NaN, slo >= shi, slo < sshift < shi, sshift < 0 or NaN; -44 for a
 * row-partitioned operator; shi = NaN takes primme_amd_svds_operator_norm_bound = sqrt(|A|_1 |A|_inf) >= sigma_max.
 * primme_svds->preconditioner = the operator handle, which owns the scratch panels; blocks wider than 8 go in chunks of 8.
 * For the real-equivalent form of a complex matrix (set_complex) the recurrence runs unchanged on the 2n / 2m real rows.
 * The products inside are not numMatvecs: primme_amd_chebyshev_stats counts them, one per vector and application of A or A'
 * (2 (steps - 1) in the normal-equation modes, 4 (steps - 1) + 2 in the augmented one).  PRIMME_AMD_CHEB_UNFUSED /
 * PRIMME_AMD_CHEB_FUSED as in primme_amd.h. */
int primme_amd_svds_operator_set_chebyshev(primme_amd_svds_operator *op, int steps, double slo, double shi, double sshift);
int primme_amd_svds_operator_norm_bound(primme_amd_svds_operator *op, double *bound);
void primme_amd_svds_chebyshev_precond(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy, int *blockSize,
      int *mode, struct primme_svds_params *ps, int *ierr);

#ifdef __cplusplus
}
#endif
#endif
