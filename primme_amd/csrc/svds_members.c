/* svds_members.c — primme_svds_params by label and by name, and its configuration listing: the tables for the engine of
 * eigs_members.c (members.h).  Behaviour restated from reference src/svds/primme_svds_interface.c:421-515 and :575-1312. */
#include "members.h"

#define AT(path) offsetof(primme_svds_params, path)
#define M(label, path, kind, arity, flags, en) {PRIMME_SVDS_##label, #label, #path, AT(path), kind, arity, flags, en}
static const pa_member svds_members[] = {
   /* the two eigensolver blocks: their address can be read, to go on with primme_get_member / primme_set_member */
   M(primme, primme, PA_MK_NESTED, 1, 0, 0),
   M(primmeStage2, primmeStage2, PA_MK_NESTED, 1, 0, 0),
   M(m, m, PA_MK_LONG, 1, 0, 0),
   M(n, n, PA_MK_LONG, 1, 0, 0),
   M(matrixMatvec, matrixMatvec, PA_MK_POINTER, 1, 0, 0),
   M(matrixMatvec_type, matrixMatvec_type, PA_MK_ENUM, 1, 0, 0),
   M(applyPreconditioner, applyPreconditioner, PA_MK_POINTER, 1, 0, 0),
   M(applyPreconditioner_type, applyPreconditioner_type, PA_MK_ENUM, 1, 0, 0),
   M(numProcs, numProcs, PA_MK_INT, 1, 0, 0),
   M(procID, procID, PA_MK_INT, 1, 0, 0),
   M(mLocal, mLocal, PA_MK_LONG, 1, 0, 0),
   M(nLocal, nLocal, PA_MK_LONG, 1, 0, 0),
   /* the preset methods are no member: the reference answers for them under the label of commInfo */
   M(commInfo, commInfo, PA_MK_POINTER, 1, 0, PA_EN_SVDS_METHOD),
   M(globalSumReal, globalSumReal, PA_MK_POINTER, 1, 0, 0),
   M(globalSumReal_type, globalSumReal_type, PA_MK_ENUM, 1, 0, 0),
   M(broadcastReal, broadcastReal, PA_MK_POINTER, 1, 0, 0),
   M(broadcastReal_type, broadcastReal_type, PA_MK_ENUM, 1, 0, 0),
   M(internalPrecision, internalPrecision, PA_MK_ENUM, 1, 0, 0),
   M(numSvals, numSvals, PA_MK_INT, 1, 0, 0),
   M(target, target, PA_MK_ENUM, 1, 0, PA_EN_SVDS_TARGET),
   M(numTargetShifts, numTargetShifts, PA_MK_INT, 1, 0, 0),
   M(targetShifts, targetShifts, PA_MK_DARRAY, 0, 0, 0),
   M(method, method, PA_MK_ENUM, 1, 0, PA_EN_SVDS_OPERATOR),
   M(methodStage2, methodStage2, PA_MK_ENUM, 1, 0, PA_EN_SVDS_OPERATOR),
   M(matrix, matrix, PA_MK_POINTER, 1, 0, 0),
   M(preconditioner, preconditioner, PA_MK_POINTER, 1, 0, 0),
   M(locking, locking, PA_MK_INT, 1, 0, 0),
   M(numOrthoConst, numOrthoConst, PA_MK_INT, 1, 0, 0),
   M(aNorm, aNorm, PA_MK_DOUBLE, 1, 0, 0),
   M(eps, eps, PA_MK_DOUBLE, 1, 0, 0),
   M(precondition, precondition, PA_MK_INT, 1, 0, 0),
   M(initSize, initSize, PA_MK_INT, 1, 0, 0),
   M(maxBasisSize, maxBasisSize, PA_MK_INT, 1, 0, 0),
   M(maxBlockSize, maxBlockSize, PA_MK_INT, 1, 0, 0),
   M(maxMatvecs, maxMatvecs, PA_MK_LONG, 1, 0, 0),
   M(iseed, iseed, PA_MK_LONG4, 1, 0, 0),      /* four values move; the arity reported is the reference's 1 */
   M(printLevel, printLevel, PA_MK_INT, 1, 0, 0),
   M(outputFile, outputFile, PA_MK_POINTER, 1, 0, 0),
   M(stats_numOuterIterations, stats.numOuterIterations, PA_MK_LONG, 1, 0, 0),
   M(stats_numRestarts, stats.numRestarts, PA_MK_LONG, 1, 0, 0),
   M(stats_numMatvecs, stats.numMatvecs, PA_MK_LONG, 1, 0, 0),
   M(stats_numPreconds, stats.numPreconds, PA_MK_LONG, 1, 0, 0),
   M(stats_numGlobalSum, stats.numGlobalSum, PA_MK_LONG, 1, PA_MF_NO_SET, 0),
   M(stats_volumeGlobalSum, stats.volumeGlobalSum, PA_MK_LONG, 1, 0, 0),
   M(stats_numBroadcast, stats.numBroadcast, PA_MK_LONG, 1, PA_MF_NO_SET, 0),
   M(stats_volumeBroadcast, stats.volumeBroadcast, PA_MK_LONG, 1, 0, 0),
   M(stats_numOrthoInnerProds, stats.numOrthoInnerProds, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_elapsedTime, stats.elapsedTime, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_timeMatvec, stats.timeMatvec, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_timePrecond, stats.timePrecond, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_timeOrtho, stats.timeOrtho, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_timeGlobalSum, stats.timeGlobalSum, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_timeBroadcast, stats.timeBroadcast, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_lockingIssue, stats.lockingIssue, PA_MK_LONG, 1, PA_MF_NO_SET, 0),
   M(convTestFun, convTestFun, PA_MK_POINTER, 1, 0, 0),
   M(convTestFun_type, convTestFun_type, PA_MK_ENUM, 1, 0, 0),
   M(convtest, convtest, PA_MK_POINTER, 1, 0, 0),
   M(monitorFun, monitorFun, PA_MK_POINTER, 1, 0, 0),
   M(monitorFun_type, monitorFun_type, PA_MK_ENUM, 1, 0, 0),
   M(monitor, monitor, PA_MK_POINTER, 1, 0, 0),
   M(queue, queue, PA_MK_POINTER, 1, 0, 0),
   M(profile, profile, PA_MK_STRING, 1, 0, 0),
};
#undef M
#undef AT
#define SVDS_ROWS ((int)(sizeof(svds_members) / sizeof(svds_members[0])))

#define K(name, en) {#name, (int)name, en, 0}
#define K_SILENT(name, en) {#name, (int)name, en, 1}
static const pa_constant svds_constants[] = {
   K(primme_svds_default, PA_EN_SVDS_METHOD), K(primme_svds_hybrid, PA_EN_SVDS_METHOD),
   K(primme_svds_normalequations, PA_EN_SVDS_METHOD), K(primme_svds_augmented, PA_EN_SVDS_METHOD),
   K(primme_svds_largest, PA_EN_SVDS_TARGET), K(primme_svds_smallest, PA_EN_SVDS_TARGET),
   K(primme_svds_closest_abs, PA_EN_SVDS_TARGET),
   K(primme_svds_op_none, PA_EN_SVDS_OPERATOR), K(primme_svds_op_AtA, PA_EN_SVDS_OPERATOR),
   K(primme_svds_op_AAt, PA_EN_SVDS_OPERATOR), K(primme_svds_op_augmented, PA_EN_SVDS_OPERATOR),
   /* for the listing of internalPrecision (no svds member answers ?_enum_member_info with these) */
   K_SILENT(primme_op_default, PA_EN_OP), K(primme_op_half, PA_EN_OP), K(primme_op_float, PA_EN_OP), K(primme_op_double, PA_EN_OP),
   K(primme_op_quad, PA_EN_OP), K_SILENT(primme_op_int, PA_EN_OP),
};
#define SVDS_CONSTANTS ((int)(sizeof(svds_constants) / sizeof(svds_constants[0])))

#define RULE "// ---------------------------------------------------\n"
#define L(style, label, aux) {style, PRIMME_SVDS_##label, aux, NULL}
#define TEXT(t) {PA_DS_TEXT, 0, 0, t}
static const pa_display_line svds_listing[] = {
   TEXT(RULE "//            primme_svds configuration               \n" RULE),
   L(PA_DS_INT, m, 0), L(PA_DS_INT, n, 0), L(PA_DS_INT, mLocal, 0), L(PA_DS_INT, nLocal, 0), L(PA_DS_INT, numProcs, 0),
   L(PA_DS_INT, procID, 0),
   TEXT("\n// Output and reporting\n"),
   L(PA_DS_INT, printLevel, 0),
   TEXT("\n// Solver parameters\n"),
   L(PA_DS_INT, numSvals, 0), L(PA_DS_E, aNorm, 0), L(PA_DS_E, eps, 0), L(PA_DS_INT, maxBasisSize, 0),
   L(PA_DS_INT, maxBlockSize, 0), L(PA_DS_INT, maxMatvecs, 0),
   L(PA_DS_ENUM, target, PA_EN_SVDS_TARGET),
   L(PA_DS_INT, numTargetShifts, 0), L(PA_DS_SHIFTS, targetShifts, PRIMME_SVDS_numTargetShifts),
   L(PA_DS_INT, locking, 0), L(PA_DS_INT, initSize, 0), L(PA_DS_INT, numOrthoConst, 0), L(PA_DS_SEED, iseed, 0),
   L(PA_DS_INT, precondition, 0),
   L(PA_DS_ENUM, method, PA_EN_SVDS_OPERATOR), L(PA_DS_ENUM, methodStage2, PA_EN_SVDS_OPERATOR),
   L(PA_DS_ENUM, internalPrecision, PA_EN_OP),
};

void primme_svds_display_params(primme_svds_params primme_svds) {
   FILE *out = primme_svds.outputFile;
   pa_display(out, "primme_svds", svds_members, SVDS_ROWS, &primme_svds, svds_listing,
         (int)(sizeof(svds_listing) / sizeof(svds_listing[0])), svds_constants, SVDS_CONSTANTS);
   if (primme_svds.method != primme_svds_op_none) {
      fputs("\n" RULE "//            1st stage primme configuration          \n" RULE, out);
      pa_display_eigs(out, "primme", &primme_svds.primme);
   }
   if (primme_svds.methodStage2 != primme_svds_op_none) {
      fputs("\n" RULE "//            2st stage primme configuration          \n" RULE, out);
      pa_display_eigs(out, "primmeStage2", &primme_svds.primmeStage2);
   }
   fflush(out);
}

int primme_svds_get_member(primme_svds_params *primme_svds, primme_svds_params_label label, void *value) {
   return pa_member_get(svds_members, SVDS_ROWS, primme_svds, (int)label, value);
}

int primme_svds_set_member(primme_svds_params *primme_svds, primme_svds_params_label label, void *value) {
   return pa_member_set(svds_members, SVDS_ROWS, primme_svds, (int)label, value);
}

int primme_svds_member_info(primme_svds_params_label *label, const char **label_name, primme_type *type, int *arity) {
   int l = label ? (int)*label : 0;
   const int rc = pa_member_info(svds_members, SVDS_ROWS, label ? &l : NULL, label_name, type, arity);
   if (label) *label = (primme_svds_params_label)l;
   return rc;
}

int primme_svds_constant_info(const char *label_name, int *value) {
   if (pa_constant_info(svds_constants, SVDS_CONSTANTS, label_name, value) == 0) return 0;
   return primme_constant_info(label_name, value);
}

int primme_svds_enum_member_info(primme_svds_params_label label, int *value, const char **value_name) {
   return pa_enum_member_info(svds_members, SVDS_ROWS, svds_constants, SVDS_CONSTANTS, (int)label, value, value_name);
}
