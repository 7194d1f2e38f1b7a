/* primme_amd.h — public solver ABI of the MI355X-native Davidson/GD+k path.
 *
 * This is boundary B1 of SURVEY.md §8(b): the structs, enums and entry points a
 * caller of the reference's eigensolver binds to.  A program written against the
 * reference's GPU flavour (cublas_dprimme: device `evecs`, device pointers handed
 * to matrixMatvec, host evals/resNorms — reference examples/ex_eigs_dhipblas.c:174-182,
 * :239-264) switches to this library by calling hip_dprimme() instead.
 *
 * LAYOUT IS ABI.  Field order, widths and enum values below reproduce
 * reference include/primme_eigs.h:47-253 (sizeof(primme_params) == 640,
 * sizeof(primme_stats) == 200 on x86-64; tests/test_abi_and_params.py checks every offset
 * against the table captured from the reference build).  Only declarations are
 * shared; every definition in this repository is new code.
 */
#ifndef PRIMME_AMD_H
#define PRIMME_AMD_H

#include <stdint.h>
#include <stdio.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef PRIMME_INT
#define PRIMME_INT int64_t /* reference include/primme.h:82-87 */
#endif

/* ---- return codes (reference include/primme.h:116-123; -4..-39 are the
 *      argument checks of reference src/eigs/primme_c.c:438-535) ------------- */
#define PRIMME_UNEXPECTED_FAILURE   (-1)
#define PRIMME_MALLOC_FAILURE       (-2)
#define PRIMME_MAIN_ITER_FAILURE    (-3)
#define PRIMME_LAPACK_FAILURE       (-40)
#define PRIMME_USER_FAILURE         (-41)
#define PRIMME_ORTHO_CONST_FAILURE  (-42)
#define PRIMME_PARALLEL_FAILURE     (-43)
#define PRIMME_FUNCTION_UNAVAILABLE (-44)

/* ---- enums: values are ABI (reference include/primme_eigs.h:47-107) --------- */
typedef enum {
   primme_smallest = 0, primme_largest, primme_closest_geq, primme_closest_leq,
   primme_closest_abs, primme_largest_abs
} primme_target;

typedef enum {
   primme_proj_default = 0, primme_proj_RR, primme_proj_harmonic, primme_proj_refined
} primme_projection;

typedef enum {
   primme_init_default = 0, primme_init_krylov, primme_init_random, primme_init_user
} primme_init;

typedef enum {
   primme_full_LTolerance = 0, primme_decreasing_LTolerance,
   primme_adaptive_ETolerance, primme_adaptive
} primme_convergencetest;

typedef enum {
   primme_event_outer_iteration = 0, primme_event_inner_iteration, primme_event_restart,
   primme_event_reset, primme_event_converged, primme_event_locked,
   primme_event_message, primme_event_profile
} primme_event;

typedef enum {
   primme_orth_default = 0, primme_orth_implicit_I, primme_orth_explicit_I
} primme_orth;

typedef enum {
   primme_op_default = 0, primme_op_half, primme_op_float, primme_op_double,
   primme_op_quad, primme_op_int
} primme_op_datatype;

/* ---- counters (reference include/primme_eigs.h:109-135) --------------------- */
typedef struct primme_stats {
   PRIMME_INT numOuterIterations, numRestarts, numMatvecs, numPreconds;
   PRIMME_INT numGlobalSum, numBroadcast, volumeGlobalSum, volumeBroadcast;
   double flopsDense;          /* flops of the fused Ritz/residual panel updates   */
   double numOrthoInnerProds;  /* one per basis column touched by the orthogonaliser */
   double elapsedTime, timeMatvec, timePrecond, timeOrtho, timeGlobalSum,
          timeBroadcast, timeDense;
   double estimateMinEVal, estimateMaxEVal, estimateLargestSVal;
   double estimateBNorm, estimateInvBNorm;
   double maxConvTol;             /* largest residual norm among locked pairs */
   double estimateResidualError;  /* accumulated error in V, W                */
   PRIMME_INT lockingIssue;
} primme_stats;

typedef struct JD_projectors { int LeftQ, LeftX, RightQ, RightX, SkewQ, SkewX; } JD_projectors;
typedef struct projection_params { primme_projection projection; } projection_params;
typedef struct correction_params {
   int precondition, robustShifts, maxInnerIterations;
   struct JD_projectors projectors;
   primme_convergencetest convTest;
   double relTolBase;
} correction_params;
typedef struct restarting_params { int maxPrevRetain; } restarting_params;

struct primme_params;
/* Block operator callback: y(:,0:bs) = Op * x(:,0:bs); everything by pointer,
 * *ierr != 0 aborts the solve with PRIMME_USER_FAILURE
 * (reference include/primme_eigs.h:170-185, src/eigs/auxiliary_eigs.c:183-230).
 * In hip_?primme x and y are DEVICE pointers, ld = ldOPs. */
typedef void (*primme_block_op)(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy,
      int *blockSize, struct primme_params *primme, int *ierr);

/* ---- the parameter block (reference include/primme_eigs.h:166-253) ---------- */
typedef struct primme_params {
   PRIMME_INT n;
   primme_block_op matrixMatvec;        primme_op_datatype matrixMatvec_type;
   primme_block_op applyPreconditioner; primme_op_datatype applyPreconditioner_type;
   primme_block_op massMatrixMatvec;    primme_op_datatype massMatrixMatvec_type;

   /* row partition (reference :187-198, examples/ex_eigs_mpi.c:100-123) */
   int numProcs, procID;
   PRIMME_INT nLocal;
   void *commInfo;
   void (*globalSumReal)(void *sendBuf, void *recvBuf, int *count,
         struct primme_params *primme, int *ierr);
   primme_op_datatype globalSumReal_type;
   void (*broadcastReal)(void *buffer, int *count, struct primme_params *primme, int *ierr);
   primme_op_datatype broadcastReal_type;

   int numEvals;
   primme_target target;
   int numTargetShifts;
   double *targetShifts;

   int dynamicMethodSwitch, locking, initSize, numOrthoConst;
   int maxBasisSize, minRestartSize, maxBlockSize;
   PRIMME_INT maxMatvecs, maxOuterIterations;
   PRIMME_INT iseed[4];
   double aNorm, BNorm, invBNorm, eps;
   primme_orth orth;
   primme_op_datatype internalPrecision;

   int printLevel;
   FILE *outputFile;

   void *matrix, *preconditioner, *massMatrix;
   double *ShiftsForPreconditioner;
   primme_init initBasisMode;
   PRIMME_INT ldevecs, ldOPs;

   struct projection_params projectionParams;
   struct restarting_params restartingParams;
   struct correction_params correctionParams;
   struct primme_stats stats;

   void (*convTestFun)(double *eval, void *evec, double *rNorm, int *isconv,
         struct primme_params *primme, int *ierr);
   primme_op_datatype convTestFun_type;
   void *convtest;
   void (*monitorFun)(void *basisEvals, int *basisSize, int *basisFlags, int *iblock,
         int *blockSize, void *basisNorms, int *numConverged, void *lockedEvals,
         int *numLocked, int *lockedFlags, void *lockedNorms, int *inner_its,
         void *LSRes, const char *msg, double *time, primme_event *event,
         struct primme_params *primme, int *err);
   primme_op_datatype monitorFun_type;
   void *monitor;
   void *queue;          /* hip_?primme: optional hipStream_t* (NULL = library stream) */
   const char *profile;
} primme_params;

typedef enum {
   PRIMME_DEFAULT_METHOD = 0, PRIMME_DYNAMIC, PRIMME_DEFAULT_MIN_TIME,
   PRIMME_DEFAULT_MIN_MATVECS, PRIMME_Arnoldi, PRIMME_GD, PRIMME_GD_plusK,
   PRIMME_GD_Olsen_plusK, PRIMME_JD_Olsen_plusK, PRIMME_RQI, PRIMME_JDQR,
   PRIMME_JDQMR, PRIMME_JDQMR_ETol, PRIMME_STEEPEST_DESCENT,
   PRIMME_LOBPCG_OrthoBasis, PRIMME_LOBPCG_OrthoBasis_Window
} primme_preset_method;

/* ---- access to the members by label or by name: what the bindings of the reference and its Fortran layer are written on
 *      (reference include/primme_eigs.h:279-378; the numeric values are ABI, bindings pass them as integers) ---------------- */
typedef enum { primme_int = 0, primme_double, primme_pointer, primme_string } primme_type;

typedef enum {
   PRIMME_invalid_label = 0,
   PRIMME_n = 1, PRIMME_matrixMatvec = 2, PRIMME_matrixMatvec_type = 3, PRIMME_applyPreconditioner = 4,
   PRIMME_applyPreconditioner_type = 5, PRIMME_massMatrixMatvec = 6, PRIMME_massMatrixMatvec_type = 7, PRIMME_numProcs = 8,
   PRIMME_procID = 9, PRIMME_commInfo = 10, PRIMME_nLocal = 11, PRIMME_globalSumReal = 12, PRIMME_globalSumReal_type = 13,
   PRIMME_broadcastReal = 14, PRIMME_broadcastReal_type = 15, PRIMME_numEvals = 16, PRIMME_target = 17,
   PRIMME_numTargetShifts = 18, PRIMME_targetShifts = 19, PRIMME_locking = 20, PRIMME_initSize = 21,
   PRIMME_numOrthoConst = 22, PRIMME_maxBasisSize = 23, PRIMME_minRestartSize = 24, PRIMME_maxBlockSize = 25,
   PRIMME_maxMatvecs = 26, PRIMME_maxOuterIterations = 27, PRIMME_iseed = 28, PRIMME_aNorm = 29, PRIMME_BNorm = 30,
   PRIMME_invBNorm = 31, PRIMME_eps = 32, PRIMME_orth = 33, PRIMME_internalPrecision = 34, PRIMME_printLevel = 35,
   PRIMME_outputFile = 36, PRIMME_matrix = 37, PRIMME_massMatrix = 38, PRIMME_preconditioner = 39,
   PRIMME_ShiftsForPreconditioner = 40, PRIMME_initBasisMode = 41, PRIMME_projectionParams_projection = 42,
   PRIMME_restartingParams_maxPrevRetain = 43, PRIMME_correctionParams_precondition = 44,
   PRIMME_correctionParams_robustShifts = 45, PRIMME_correctionParams_maxInnerIterations = 46,
   PRIMME_correctionParams_projectors_LeftQ = 47, PRIMME_correctionParams_projectors_LeftX = 48,
   PRIMME_correctionParams_projectors_RightQ = 49, PRIMME_correctionParams_projectors_RightX = 50,
   PRIMME_correctionParams_projectors_SkewQ = 51, PRIMME_correctionParams_projectors_SkewX = 52,
   PRIMME_correctionParams_convTest = 53, PRIMME_correctionParams_relTolBase = 54, PRIMME_stats_numOuterIterations = 55,
   PRIMME_stats_numRestarts = 56, PRIMME_stats_numMatvecs = 57, PRIMME_stats_numPreconds = 58,
   PRIMME_stats_numGlobalSum = 59, PRIMME_stats_volumeGlobalSum = 60, PRIMME_stats_numBroadcast = 61,
   PRIMME_stats_volumeBroadcast = 62, PRIMME_stats_flopsDense = 63, PRIMME_stats_numOrthoInnerProds = 64,
   PRIMME_stats_elapsedTime = 65, PRIMME_stats_timeMatvec = 66, PRIMME_stats_timePrecond = 67, PRIMME_stats_timeOrtho = 68,
   PRIMME_stats_timeGlobalSum = 69, PRIMME_stats_timeBroadcast = 70, PRIMME_stats_timeDense = 71,
   PRIMME_stats_estimateMinEVal = 72, PRIMME_stats_estimateMaxEVal = 73, PRIMME_stats_estimateLargestSVal = 74,
   PRIMME_stats_estimateBNorm = 75, PRIMME_stats_estimateInvBNorm = 76, PRIMME_stats_maxConvTol = 77,
   PRIMME_stats_lockingIssue = 78, PRIMME_dynamicMethodSwitch = 79, PRIMME_convTestFun = 80, PRIMME_convTestFun_type = 81,
   PRIMME_convtest = 82, PRIMME_ldevecs = 83, PRIMME_ldOPs = 84, PRIMME_monitorFun = 85, PRIMME_monitorFun_type = 86,
   PRIMME_monitor = 87, PRIMME_queue = 88, PRIMME_profile = 89
} primme_params_label;

/* convergence flags reported to monitorFun (reference src/eigs/common_eigs.h:41-46) */
enum primme_amd_conv_flags {
   PRIMME_AMD_UNCONVERGED = 0, PRIMME_AMD_SKIP_UNTIL_RESTART, PRIMME_AMD_CONVERGED,
   PRIMME_AMD_PRACTICALLY_CONVERGED
};

/* ---- entry points ----------------------------------------------------------- */
/* reference src/eigs/primme_interface.c:101, :293, :543, :228 */
void primme_initialize(primme_params *primme);
int  primme_set_method(primme_preset_method method, primme_params *primme);
void primme_set_defaults(primme_params *primme);
void primme_free(primme_params *primme);
primme_params *primme_params_create(void);
int  primme_params_destroy(primme_params *primme);

/* Prints the configuration to primme.outputFile, in the reference's format character for character (the block is passed
 * by value, reference src/eigs/primme_interface.c:629). */
void primme_display_params(primme_params primme);
/* Members by label.  `value` is, by the member's kind (primme_member_info): primme_int -> PRIMME_INT* (iseed: 4 of them),
 * primme_double with arity 1 -> double*; get stores through it, set reads through it.  For primme_pointer, primme_string and
 * the arrays of arity 0 (targetShifts, ShiftsForPreconditioner) set takes the pointer to store AS `value` and get stores the
 * member through (void **)value.  Return 0, or 1 for an unknown label, a value above INT_MAX for an int member, or a member
 * the reference does not serve: get of globalSumReal_type / broadcastReal_type, set of stats_numGlobalSum /
 * stats_numBroadcast.  Those two *_type labels have no name either: primme_member_info returns 1 for them. */
int primme_get_member(primme_params *primme, primme_params_label label, void *value);
int primme_set_member(primme_params *primme, primme_params_label label, void *value);
/* Looks a member up by *label, or by *label_name when that is given and matches (names join the nested structures with '_'
 * and drop "Params": correction_maxInnerIterations); fills in the other of the two, the kind and the arity.  Any of the
 * pointers may be NULL except both of label and label_name.  Returns 0, or 1 when nothing matches. */
int primme_member_info(primme_params_label *label, const char **label_name, primme_type *type, int *arity);
/* The value of an enumerator given by name ("primme_proj_refined", "PRIMME_JDQMR"); 0, or 1 for an unknown name. */
int primme_constant_info(const char *label_name, int *value);
/* Enumerators of the member `label`: *value >= 0 and *value_name == NULL asks for the name, *value < 0 and a name asks for the
 * value.  0; -1 for any other combination; -2 when not found or the member is not of an enumeration the reference lists
 * (it lists target, projection, initBasisMode, convTest, orth and five of the *_type members; the preset methods answer
 * to the label PRIMME_commInfo). */
int primme_enum_member_info(primme_params_label label, int *value, const char **value_name);

/* Solvers: same contract as the reference's cublas_?primme / magma_?primme
 * (reference include/primme_eigs.h:394-417, src/eigs/primme_c.c:103-108):
 *   evals[numEvals], resNorms[numEvals]   HOST arrays
 *   evecs[ldevecs*(numOrthoConst+max(numEvals,initSize))]  DEVICE array, column-major;
 *        on input: numOrthoConst constraint vectors then initSize guesses
 *   returns 0, or <0 (codes above); primme->initSize = converged pairs returned;
 *   primme->stats filled; primme->aNorm back-filled when it was <= 0.
 * Requires the GPU: there is no CPU fallback; a missing/failed device returns
 * PRIMME_UNEXPECTED_FAILURE.
 * hip_zprimme / hip_cprimme (Hermitian problems; evecs and the callbacks' vectors are DEVICE
 * arrays of (re, im) pairs, leading dimensions in complex elements exactly as for
 * cublas_zprimme) run natively on complex panels (csrc/hipk_complex.hip, the host solver compiled
 * for double complex, csrc/eigs_*_z.c): the GD family, JDQMR and the dynamic switch, with
 * Rayleigh-Ritz, harmonic or refined extraction — zprimme's eigenpairs, residual norms and, on the
 * committed extremal fixtures, its outer-iteration / matvec / restart counts.  PRIMME_AMD_COMPLEX_REAL_FORM=1
 * (csrc/eigs_complex.c) selects the real-equivalent 2n form instead: same eigenpairs, about
 * twice the operator applications; kept as a cross-check. */
int hip_dprimme(double *evals, double *evecs, double *resNorms, primme_params *primme);
int hip_zprimme(double *evals, void *evecs, double *resNorms, primme_params *primme);
int hip_sprimme(float *evals, float *evecs, float *resNorms, primme_params *primme);
int hip_cprimme(float *evals, void *evecs, float *resNorms, primme_params *primme);

/* The reference's CPU entry points with their HOST-pointer contract (include/primme_eigs.h:386-393,
 * src/eigs/primme_c.c:103-108): evecs is a host array [constraints | guesses], the callbacks get host
 * pointers with leading dimension ldOPs, primme->queue must be NULL.  A program written against the
 * CPU library (examples/ex_eigs_dseq.c) relinks unchanged; the solve runs on the device and every
 * operator application is staged through pinned host memory (csrc/eigs_hostapi.c), so this is the
 * plumbing path — use hip_?primme with a device callback for the device rate. */
int dprimme(double *evals, double *evecs, double *resNorms, primme_params *primme);
int zprimme(double *evals, void *evecs, double *resNorms, primme_params *primme);
int sprimme(float *evals, float *evecs, float *resNorms, primme_params *primme);
int cprimme(float *evals, void *evecs, float *resNorms, primme_params *primme);

/* ---- ready-made callbacks (what examples/ex_eigs_dhipblas.c:239-264 and
 *      examples/ex_eigs_mpi.c:209-218 hand-write for every application) ------- */

/* matrixMatvec for a device CSR matrix: set primme->matrix = handle returned by
 * primme_amd_operator_create() over a hipk_csr_create() / hipk_stencil_create() matrix
 * (primme_amd_comm.h, primme_amd_kernels.h). */
void primme_amd_matvec(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy, int *blockSize,
      struct primme_params *primme, int *ierr);
/* massMatrixMatvec for a device CSR mass matrix B of a generalised problem A x = lambda B x (round 6; reference
 * primme_eigs.h:182-185, auxiliary_eigs.c:250-290): set primme->massMatrix = another operator handle. */
void primme_amd_mass_matvec(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy, int *blockSize,
      struct primme_params *primme, int *ierr);
/* Jacobi (diagonal) preconditioner y = (diag(A) - shift)^-1 x with the shifts the
 * solver publishes in primme->ShiftsForPreconditioner; primme->preconditioner =
 * the same operator handle, flavour chosen with
 * primme_amd_operator_set_jacobi() (cf. reference tests/COMMON/mat.c
 * createInvDiagPrecNative / examples/ex_eigs_dseq.c:187-202). */
void primme_amd_jacobi_precond(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy,
      int *blockSize, struct primme_params *primme, int *ierr);
/* Chebyshev polynomial preconditioner y = p(A) x: the `steps`-th iterate of Chebyshev iteration for (A - sigma I) y = x
 * started from y = 0, which damps the part [lo, hi] of the spectrum (steps - 1 applications of the operator per vector; no
 * reference counterpart).  primme->preconditioner = the operator handle, configured with
 *    primme_amd_operator_set_chebyshev(op, steps, lo, hi, fixed, shift)
 * fixed = 1: sigma = shift, which must not lie inside (lo, hi).  fixed = 0: column c uses primme->ShiftsForPreconditioner[c],
 * kept at or below lo for primme_smallest and at or above hi for primme_largest; any other target makes the callback set
 * *ierr = 1.  hi = NaN: the Gershgorin upper bound of the operator (primme_amd_operator_gershgorin; collective when the
 * operator is row-partitioned).  Returns -1 for steps < 1, lo = NaN, lo >= hi or a fixed shift inside the interval.
 * lo is the upper end of what is WANTED (for the smallest eigenvalues: anything in the gap above them, e.g. a Ritz value
 * of a coarse run).  hi must bound the spectrum: p grows without limit on (hi, lambda_max], the preconditioner is then bad
 * (nothing faults).  Block columns beyond 8 are processed in chunks; the operator owns the scratch panels.
 * PRIMME_AMD_CHEB_UNFUSED=1 (read by primme_amd_operator_set_chebyshev) keeps the operator product and the recurrence in
 * separate launches for every operator (A/B measurements); by default single-rank real CSR operators run both in one pass.
 * The applications of the operator inside the preconditioner are not counted in stats.numMatvecs (the reference does not
 * count work inside a user preconditioner either); primme_amd_chebyshev_stats returns, for this process since the last
 * call, the vectors preconditioned, the operator products (vectors) spent on them and how many of those ran fused. */
struct primme_amd_operator;
int primme_amd_operator_set_chebyshev(struct primme_amd_operator *op, int steps, double lo, double hi, int fixed, double shift);
int primme_amd_operator_gershgorin(struct primme_amd_operator *op, double *lo, double *hi);
void primme_amd_chebyshev_precond(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy,
      int *blockSize, struct primme_params *primme, int *ierr);
void primme_amd_chebyshev_stats(long *applies, long *operator_products, long *fused_steps);
/* Geometric multigrid preconditioner for grid Laplacians (no reference counterpart): y = K^-1 x is ONE
 * symmetric V(smooth_steps, smooth_steps) cycle from a zero start for
 *    M = scale L + shift I,
 * L the Dirichlet Laplacian of the nx x ny x nz grid that hipk_stencil_create represents (x fastest, off-diagonals -1, diagonal
 * 2 per dimension with more than one point).  K does not follow the solver's shifts and is symmetric positive definite, whatever
 * the operator of the eigenproblem is: the stencil form, a CSR Laplacian, or -Laplacian + V with shift about the mean of V.
 *    primme_amd_operator_set_multigrid(op, nx, ny, nz, smooth_steps, coarse_steps, scale, shift)
 * then primme->preconditioner = the operator handle and primme->applyPreconditioner = primme_amd_multigrid_precond.
 * Levels: primme_amd_mg_plan (level 0 = the grid with weights 1; a dimension of 3 or more points is halved, coarse point j on
 * fine point 2 j + 1, its weight divided by 4; the last level has no such dimension or at most PRIMME_AMD_MG_COARSE_POINTS
 * points).  Level operator M_l = scale sum_d w_l,d L_d + shift I (rediscretised).  Transfers: tensor products of 1-D linear
 * interpolation P_d (identity in a dimension that is kept) and R_d = P_d' / 2.  Smoother: smooth_steps steps of the Chebyshev
 * iteration for M_l on [hi_l / (2 D_l), hi_l], hi_l the exact largest eigenvalue and D_l the number of dimensions with more
 * than one point, the same polynomial before (from zero) and after (from the corrected iterate) the coarse correction.  Last
 * level: coarse_steps Chebyshev steps over its exact spectrum.  Kernels: csrc/hipk_mg.hip.
 * set_multigrid returns -44 for a row-partitioned operator, a complex operator or the real-equivalent mode, -1 for nx ny nz !=
 * the operator's rows, steps < 1, scale <= 0, shift < 0 (or a singular M: one grid point and shift = 0).  The level scratch is
 * allocated at the first application and freed with the operator; block columns beyond 8 are processed in chunks.
 * primme_amd_multigrid_stats: for this process since the last call, the vectors preconditioned and the kernel launches. */
#define PRIMME_AMD_MG_MAXLEVELS 24
#define PRIMME_AMD_MG_COARSE_POINTS 32
int primme_amd_mg_plan(const int dims[3], int *nlevels, int n[][3], double w[][3]);
int primme_amd_operator_set_multigrid(struct primme_amd_operator *op, int nx, int ny, int nz, int smooth_steps, int coarse_steps,
      double scale, double shift);
void primme_amd_multigrid_precond(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy,
      int *blockSize, struct primme_params *primme, int *ierr);
void primme_amd_multigrid_stats(long *applies, long *launches);
/* Aggregation algebraic multigrid preconditioner for CSR operators (no reference counterpart): y = K^-1 x
 * is ONE symmetric V(smooth_steps, smooth_steps) cycle from a zero start for M = A + shift I, A the operator's own SYMMETRIC
 * CSR matrix (a positive diagonal; symmetry is the caller's promise), shift >= 0.  The hierarchy is built on the host from the
 * CSR arrays handed over (the ones the operator was created from, values in the operator's dtype) by plain aggregation
 * (primme_amd_amg_plan_create in primme_amd_io.h: strength threshold theta, Galerkin coarse matrices), uploaded, and the host
 * copy freed.  K does not follow the solver's shifts and is symmetric positive definite: GD+k, JDQMR and the generalised
 * problems take it.
 *    primme_amd_operator_set_amg(op, rowptr_host, colind_host, values_host, smooth_steps, coarse_steps, theta, over, shift)
 *    (usual values 2, 16, 0.08, 1.0, 0.0), then primme->preconditioner = the operator handle and
 *    primme->applyPreconditioner = primme_amd_amg_precond.
 * Every level but the last: smooth_steps steps of the Chebyshev iteration for D_l^-1 M_l on [rho_l / 4, rho_l] from zero, the
 * residual, its restriction (sums over the aggregates), the coarse cycle, y += over P y_c (over in [1, 2): the over-correction
 * of unsmoothed aggregation; 1 is the textbook cycle), and the same polynomial again from the corrected iterate.  Last level:
 * at most PRIMME_AMD_AMG_DENSE_ROWS rows: the dense inverse from a host Cholesky factorisation, one launch; more (the
 * aggregation stalled): coarse_steps Chebyshev steps on [rho_L / 4, rho_L].  Level 0 runs on the operator's own matrix with the
 * shift folded into the product; the other levels are hipk_csr_create handles.  Kernels: csrc/hipk_amg.hip.
 * set_amg returns -44 for a row-partitioned operator, a complex operator, the real-equivalent mode or a stencil operator (that
 * one has set_multigrid); -1 for steps < 1, theta outside [0, 1), over outside [1, 2), shift < 0, host arrays whose size
 * differs from the operator's, a plan error (a row without a positive diagonal entry) or a last level that is not positive
 * definite; the operator is then unchanged.  The scratch (4 vectors per level and column of the block, at most 8 columns) is
 * allocated at the first application and freed with the operator; block columns beyond 8 are processed in chunks.  The
 * products inside are not counted in numMatvecs.
 * primme_amd_amg_stats: for this process since the last call, the vectors preconditioned, the launches (kernels and level
 * products) and the levels of the hierarchy applied last.
 *
 * Smoothed aggregation:
 *    primme_amd_operator_set_amg_smoothed(op, rowptr_host, colind_host, values_host, smooth_steps, coarse_steps, theta, omega,
 *    shift)   (usual values 2, 16, 0.08, 4/3, 0.0), then the same two members of primme_params.
 * The hierarchy is that of primme_amd_amg_plan_create_smoothed: P_l = (I - (omega / rho_l) D_l^-1 M_l) T_l for the 0/1 matrix
 * T_l of the same aggregates and M_{l+1} = P_l' M_l P_l.  The cycle is the one above with the restriction and interpolation
 * through hipk_amg_csr_apply on P_l' and P_l, both uploaded in CSR with double values, and over = 1; K is symmetric positive
 * definite as before, since P_l' is the exact transpose and the post-smoother is the same construction.  11 launches per level
 * and chunk, like the plain cycle.  Extra device memory: about 2 nnz(P_l) 12 bytes per level (P_l and P_l', an int32 index
 * and a double per entry; nnz(P_0) is about 2.5 n for the 5-point Laplacian), besides the coarse matrices, which are denser
 * than those of plain aggregation.  Preconditions and return codes as set_amg; -1 also for omega outside (0, 2).
 * primme_amd_amg_precond and primme_amd_amg_stats serve both. */
int primme_amd_operator_set_amg_smoothed(struct primme_amd_operator *op, const int32_t *rowptr_host, const int32_t *colind_host,
      const void *values_host, int smooth_steps, int coarse_steps, double theta, double omega, double shift);
int primme_amd_operator_set_amg(struct primme_amd_operator *op, const int32_t *rowptr_host, const int32_t *colind_host,
      const void *values_host, int smooth_steps, int coarse_steps, double theta, double over, double shift);
void primme_amd_amg_precond(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy,
      int *blockSize, struct primme_params *primme, int *ierr);
void primme_amd_amg_stats(long *applies, long *launches, long *levels);
/* ---- a hierarchy of the algebraic multigrid preconditioner as an object of its own ----
 * set_amg[_smoothed] build, upload and tie a hierarchy to one operator in one call; a hierarchy made here is built once and
 * attached to as many solves and operators over the same matrix as wanted:
 *    primme_amd_amg_hierarchy_create(op, rowptr_host, colind_host, values_host, smoothed, theta, omega, shift, setup, &h);
 *    primme_amd_operator_set_amg_hierarchy(op, h, smooth_steps, coarse_steps, over);     then as after set_amg
 * values_host in the operator's type; smoothed = 0: plain aggregation (omega is not read), 1: smoothed aggregation.
 * setup = 0: the hierarchy of primme_amd_amg_plan_create[_smoothed] from the host, the very arrays set_amg[_smoothed] upload;
 * setup = 1 (smoothed only, else -44): the aggregation passes on the host, the prolongator, its transpose, the triple product,
 * 1 / diag and rho of every level on the device (csrc/hipk_amg_setup.hip), the same hierarchy up to the rounding of the coarse
 * matrices, whose sums run in another order; a level whose products would pass INT32_MAX entries or the device's memory is
 * built by the host routines instead (primme_amd_amg_hierarchy_stages counts them; the environment variable
 * PRIMME_AMD_AMG_SETUP_MAX_ENTRIES, read when a hierarchy is created, lowers that limit).  Any other value of setup returns -1.
 * The hierarchy owns the device arrays of the levels >= 1, the aggregate maps or P_l / R_l, 1 / diag and the dense inverse of
 * the last level; level 0 runs on the operator it is attached to.  smooth_steps, coarse_steps and over belong to the
 * attachment: one hierarchy serves V(1,1) and V(2,2); over must be 1 with a smoothed hierarchy.  Reference-counted: an
 * operator holds a reference while the hierarchy is attached, either side may be destroyed first, attaching another hierarchy
 * or calling set_amg* releases the one attached.  It may be attached to several operators over the same matrix, a double and a
 * float one included (the hierarchy's data is double for both).  Not thread-safe.
 * create / set_amg_hierarchy: -44 as set_amg; -1 for an argument out of range (as set_amg), a plan the host refuses, a device
 * failure, an operator whose rows or entries differ from the matrix the hierarchy was built from.
 * _info: levels, and per level (arrays of PRIMME_AMD_AMG_MAXLEVELS) the rows, the entries of M_l and of P_l; the seconds of
 * the whole create call and of the device stages in it; how often it was attached.  Any pointer may be NULL.
 * _stages: the levels that fell back to the host and seconds[PRIMME_AMD_AMG_MAXLEVELS][6] of the device set-up per level:
 * aggregation (host), P, R, triple product, finish, download of M_{l+1}.
 * _download: a host primme_amd_amg_plan (primme_amd_io.h; release with primme_amd_amg_plan_free) read back from the device
 * arrays; level 0 carries n, nnz, dinv, rho, the maps and the transfer matrices but no matrix (rowptr, colind, values NULL). */
struct primme_amd_amg_hierarchy;
struct primme_amd_amg_plan;
int primme_amd_amg_hierarchy_create(struct primme_amd_operator *op, const int32_t *rowptr_host, const int32_t *colind_host,
      const void *values_host, int smoothed, double theta, double omega, double shift, int setup, struct primme_amd_amg_hierarchy **h);
void primme_amd_amg_hierarchy_destroy(struct primme_amd_amg_hierarchy *h);
int primme_amd_operator_set_amg_hierarchy(struct primme_amd_operator *op, struct primme_amd_amg_hierarchy *h, int smooth_steps,
      int coarse_steps, double over);
int primme_amd_amg_hierarchy_info(const struct primme_amd_amg_hierarchy *h, int *nlevels, int64_t *rows, int64_t *nnz, int64_t *pnnz,
      double *setup_seconds, double *device_seconds, long *times_attached);
int primme_amd_amg_hierarchy_stages(const struct primme_amd_amg_hierarchy *h, int *fallback_levels, double *seconds);
int primme_amd_amg_hierarchy_download(const struct primme_amd_amg_hierarchy *h, struct primme_amd_amg_plan **plan);
/* globalSumReal over RCCL: set primme->commInfo = handle from primme_amd_comm_create().
 * When the solver sees this exact function installed it reduces its DEVICE partials
 * with ncclAllReduce before the (single) device->host copy; called directly it also
 * honours the reference contract on HOST buffers (send may equal recv). */
void primme_amd_global_sum(void *sendBuf, void *recvBuf, int *count,
      struct primme_params *primme, int *ierr);

/* Diagnostics of the LAST solve of this process (block size 1, GD+k family): how many outer iterations were enqueued before
 * the host had seen the previous one and how many of those the host then adopted.  No reference
 * counterpart (the reference has no device queue to run ahead of). */
void primme_amd_prelaunch_stats(long *launched, long *adopted);
/* Diagnostics of this process (JDQMR): inner QMR steps taken since the last call, and how many of them ran with ONE host
 * synchronisation (block sizes 2 .. 8 with the library's Jacobi preconditioner: DESIGN.md section 4b); the call resets both. */
void primme_amd_qmr_step_stats(long *steps, long *one_synchronisation);

#ifdef __cplusplus
}
#endif
#endif /* PRIMME_AMD_H */
