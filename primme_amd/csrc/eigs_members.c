/* eigs_members.c — primme_params by label and by name, and its configuration listing.
 *
 * Behaviour restated from reference src/eigs/primme_interface.c:629-1835 (primme_display_params, primme_get_member,
 * primme_set_member, primme_member_info, primme_constant_info, primme_enum_member_info), oddities included: they are what
 * the reference's bindings were written against.  The reference spells each routine out as a switch over the labels; here one
 * table (members.h) drives all of them, and svds_members.c brings only its own tables.
 */
#include <inttypes.h>
#include <limits.h>
#include <string.h>
#include "members.h"

/* ---- the engine ----------------------------------------------------------------------------------------------------------- */

const pa_member *pa_member_find(const pa_member *table, int rows, int label) {
   for (int i = 0; i < rows; i++)
      if (table[i].label == label) return &table[i];
   return NULL;
}

int pa_member_get(const pa_member *table, int rows, void *base, int label, void *value) {
   const pa_member *m = pa_member_find(table, rows, label);
   if (!m || (m->flags & PA_MF_NO_GET)) return 1;
   char *at = (char *)base + m->offset;
   switch (m->kind) {
   case PA_MK_INT: *(PRIMME_INT *)value = *(int *)at; break;
   /* none of the enumerations has a negative enumerator: the compilers in use give them an unsigned type, and the reference,
    * which converts the enum itself, hands back 2^32 - 1 where -1 was stored */
   case PA_MK_ENUM: *(PRIMME_INT *)value = *(unsigned int *)at; break;
   case PA_MK_LONG: *(PRIMME_INT *)value = *(PRIMME_INT *)at; break;
   case PA_MK_LONG4: memcpy(value, at, 4 * sizeof(PRIMME_INT)); break;
   case PA_MK_DOUBLE: *(double *)value = *(double *)at; break;
   case PA_MK_NESTED: *(void **)value = at; break;
   default: memcpy(value, at, sizeof(void *)); break;   /* pointers of every sort, functions among them */
   }
   return 0;
}

int pa_member_set(const pa_member *table, int rows, void *base, int label, void *value) {
   const pa_member *m = pa_member_find(table, rows, label);
   if (!m || (m->flags & PA_MF_NO_SET) || m->kind == PA_MK_NESTED) return 1;
   char *at = (char *)base + m->offset;
   switch (m->kind) {
   case PA_MK_INT:
      if (*(PRIMME_INT *)value > INT_MAX) return 1;
      *(int *)at = (int)*(PRIMME_INT *)value;
      break;
   case PA_MK_ENUM: *(int *)at = (int)*(PRIMME_INT *)value; break;
   case PA_MK_LONG: *(PRIMME_INT *)at = *(PRIMME_INT *)value; break;
   case PA_MK_LONG4: memcpy(at, value, 4 * sizeof(PRIMME_INT)); break;
   case PA_MK_DOUBLE: *(double *)at = *(double *)value; break;
   default: memcpy(at, &value, sizeof(void *)); break;  /* the pointer itself is the value */
   }
   return 0;
}

static primme_type kind_type(int kind) {
   switch (kind) {
   case PA_MK_DOUBLE:
   case PA_MK_DARRAY: return primme_double;
   case PA_MK_POINTER:
   case PA_MK_NESTED: return primme_pointer;
   case PA_MK_STRING: return primme_string;
   default: return primme_int;
   }
}

/* The first row, in the table's order, that the given name or the given label matches decides; a label without a name
 * (name == NULL) is unknown here although get / set serve it. */
int pa_member_info(const pa_member *table, int rows, int *label, const char **label_name, primme_type *type, int *arity) {
   const char *name = label_name ? *label_name : NULL;
   if (!label && !name) return 1;
   for (int i = 0; i < rows; i++) {
      const pa_member *m = &table[i];
      if (!m->name) continue;
      if (!((name && strcmp(m->name, name) == 0) || (label && *label == m->label))) continue;
      if (label) *label = m->label;
      if (label_name) *label_name = m->name;
      if (type) *type = kind_type(m->kind);
      if (arity) *arity = m->arity;
      return 0;
   }
   return 1;
}

int pa_constant_info(const pa_constant *constants, int count, const char *name, int *value) {
   for (int i = 0; i < count; i++)
      if (strcmp(constants[i].name, name) == 0) { *value = constants[i].value; return 0; }
   return 1;
}

int pa_enum_member_info(const pa_member *table, int rows, const pa_constant *constants, int count, int label, int *value,
      const char **value_name) {
   if (!value || !value_name || (*value >= 0 && *value_name) || (*value < 0 && !*value_name)) return -1;
   const pa_member *m = pa_member_find(table, rows, label);
   if (!m || m->enumeration == PA_EN_NONE) return -2;
   for (int i = 0; i < count; i++) {
      const pa_constant *c = &constants[i];
      if (c->enumeration != m->enumeration) continue;
      if (*value_name ? strcmp(c->name, *value_name) == 0 : *value == c->value) {
         *value = c->value;
         *value_name = c->name;
         return 0;
      }
   }
   return -2;
}

/* "correctionParams.projectors.LeftQ" is listed as "correction.projectors.LeftQ" */
static void print_member_name(FILE *out, const char *prefix, const char *path) {
   fprintf(out, "%s.", prefix);
   const char *cut = strstr(path, "Params.");
   if (cut) fprintf(out, "%.*s%s", (int)(cut - path), path, cut + 6);
   else fputs(path, out);
}

void pa_display(FILE *out, const char *prefix, const pa_member *table, int rows, void *base, const pa_display_line *lines,
      int nlines, const pa_constant *constants, int count) {
   for (int l = 0; l < nlines; l++) {
      const pa_display_line *ln = &lines[l];
      if (ln->style == PA_DS_TEXT) { fputs(ln->text, out); continue; }
      const pa_member *m = pa_member_find(table, rows, ln->label);
      char *at = (char *)base + m->offset;
      PRIMME_INT iv[4] = {0, 0, 0, 0};
      if (ln->style == PA_DS_INT || ln->style == PA_DS_ENUM || ln->style == PA_DS_SEED) pa_member_get(table, rows, base, ln->label, iv);
      switch (ln->style) {
      case PA_DS_INT:
         print_member_name(out, prefix, m->path);
         fprintf(out, " = %" PRId64 "\n", (int64_t)iv[0]);
         break;
      case PA_DS_E:
      case PA_DS_G:
         print_member_name(out, prefix, m->path);
         fprintf(out, ln->style == PA_DS_E ? " = %e\n" : " = %g\n", *(double *)at);
         break;
      case PA_DS_ENUM:
         for (int i = 0; i < count; i++)
            if (constants[i].enumeration == ln->aux && constants[i].value == (int)iv[0] && !constants[i].silent) {
               print_member_name(out, prefix, m->path);
               fprintf(out, " = %s\n", constants[i].name);
               break;
            }
         break;
      case PA_DS_SHIFTS: {
         PRIMME_INT cnt = 0;
         const double *d = *(double **)at;
         pa_member_get(table, rows, base, ln->aux, &cnt);
         if (cnt <= 0 || !d) break;
         print_member_name(out, prefix, m->path);
         fputs(" =", out);
         for (PRIMME_INT i = 0; i < cnt; i++) fprintf(out, " %e", d[i]);
         fputs("\n", out);
         break;
      }
      case PA_DS_SEED:
         print_member_name(out, prefix, m->path);
         fputs(" =", out);
         for (int i = 0; i < 4; i++) fprintf(out, " %" PRId64, (int64_t)iv[i]);
         fputs("\n", out);
         break;
      }
   }
}

/* ---- primme_params ---------------------------------------------------------------------------------------------------------- */

#define AT(path) offsetof(primme_params, path)
#define M(label, name, path, kind, arity, flags, en) {PRIMME_##label, name, #path, AT(path), kind, arity, flags, en}
/* In the order in which the reference's primme_member_info tries the names (dynamicMethodSwitch is out of label order). */
static const pa_member eigs_members[] = {
   M(n, "n", n, PA_MK_LONG, 1, 0, 0),
   M(matrixMatvec, "matrixMatvec", matrixMatvec, PA_MK_POINTER, 1, 0, 0),
   M(matrixMatvec_type, "matrixMatvec_type", matrixMatvec_type, PA_MK_ENUM, 1, 0, PA_EN_OP),
   M(massMatrixMatvec, "massMatrixMatvec", massMatrixMatvec, PA_MK_POINTER, 1, 0, 0),
   M(massMatrixMatvec_type, "massMatrixMatvec_type", massMatrixMatvec_type, PA_MK_ENUM, 1, 0, PA_EN_OP),
   M(applyPreconditioner, "applyPreconditioner", applyPreconditioner, PA_MK_POINTER, 1, 0, 0),
   M(applyPreconditioner_type, "applyPreconditioner_type", applyPreconditioner_type, PA_MK_ENUM, 1, 0, PA_EN_OP),
   M(numProcs, "numProcs", numProcs, PA_MK_INT, 1, 0, 0),
   M(procID, "procID", procID, PA_MK_INT, 1, 0, 0),
   /* the preset methods are no member: the reference answers for them under the label of commInfo */
   M(commInfo, "commInfo", commInfo, PA_MK_POINTER, 1, 0, PA_EN_METHOD),
   M(nLocal, "nLocal", nLocal, PA_MK_LONG, 1, 0, 0),
   M(globalSumReal, "globalSumReal", globalSumReal, PA_MK_POINTER, 1, 0, 0),
   /* can be set, cannot be read and has no name */
   M(globalSumReal_type, NULL, globalSumReal_type, PA_MK_ENUM, 1, PA_MF_NO_GET, PA_EN_OP),
   M(broadcastReal, "broadcastReal", broadcastReal, PA_MK_POINTER, 1, 0, 0),
   M(broadcastReal_type, NULL, broadcastReal_type, PA_MK_ENUM, 1, PA_MF_NO_GET, PA_EN_OP),
   M(numEvals, "numEvals", numEvals, PA_MK_INT, 1, 0, 0),
   M(target, "target", target, PA_MK_ENUM, 1, 0, PA_EN_TARGET),
   M(numTargetShifts, "numTargetShifts", numTargetShifts, PA_MK_INT, 1, 0, 0),
   M(targetShifts, "targetShifts", targetShifts, PA_MK_DARRAY, 0, 0, 0),
   M(locking, "locking", locking, PA_MK_INT, 1, 0, 0),
   M(initSize, "initSize", initSize, PA_MK_INT, 1, 0, 0),
   M(numOrthoConst, "numOrthoConst", numOrthoConst, PA_MK_INT, 1, 0, 0),
   M(dynamicMethodSwitch, "dynamicMethodSwitch", dynamicMethodSwitch, PA_MK_INT, 1, 0, 0),
   M(maxBasisSize, "maxBasisSize", maxBasisSize, PA_MK_INT, 1, 0, 0),
   M(minRestartSize, "minRestartSize", minRestartSize, PA_MK_INT, 1, 0, 0),
   M(maxBlockSize, "maxBlockSize", maxBlockSize, PA_MK_INT, 1, 0, 0),
   M(maxMatvecs, "maxMatvecs", maxMatvecs, PA_MK_LONG, 1, 0, 0),
   M(maxOuterIterations, "maxOuterIterations", maxOuterIterations, PA_MK_LONG, 1, 0, 0),
   M(iseed, "iseed", iseed, PA_MK_LONG4, 4, 0, 0),
   M(aNorm, "aNorm", aNorm, PA_MK_DOUBLE, 1, 0, 0),
   M(BNorm, "BNorm", BNorm, PA_MK_DOUBLE, 1, 0, 0),
   M(invBNorm, "invBNorm", invBNorm, PA_MK_DOUBLE, 1, 0, 0),
   M(eps, "eps", eps, PA_MK_DOUBLE, 1, 0, 0),
   M(orth, "orth", orth, PA_MK_ENUM, 1, 0, PA_EN_ORTH),
   M(internalPrecision, "internalPrecision", internalPrecision, PA_MK_ENUM, 1, 0, 0),
   M(printLevel, "printLevel", printLevel, PA_MK_INT, 1, 0, 0),
   M(outputFile, "outputFile", outputFile, PA_MK_POINTER, 1, 0, 0),
   M(matrix, "matrix", matrix, PA_MK_POINTER, 1, 0, 0),
   M(massMatrix, "massMatrix", massMatrix, PA_MK_POINTER, 1, 0, 0),
   M(preconditioner, "preconditioner", preconditioner, PA_MK_POINTER, 1, 0, 0),
   M(ShiftsForPreconditioner, "ShiftsForPreconditioner", ShiftsForPreconditioner, PA_MK_DARRAY, 0, 0, 0),
   M(initBasisMode, "initBasisMode", initBasisMode, PA_MK_ENUM, 1, 0, PA_EN_INIT),
   M(projectionParams_projection, "projection_projection", projectionParams.projection, PA_MK_ENUM, 1, 0, PA_EN_PROJECTION),
   M(restartingParams_maxPrevRetain, "restarting_maxPrevRetain", restartingParams.maxPrevRetain, PA_MK_INT, 1, 0, 0),
   M(correctionParams_precondition, "correction_precondition", correctionParams.precondition, PA_MK_INT, 1, 0, 0),
   M(correctionParams_robustShifts, "correction_robustShifts", correctionParams.robustShifts, PA_MK_INT, 1, 0, 0),
   M(correctionParams_maxInnerIterations, "correction_maxInnerIterations", correctionParams.maxInnerIterations, PA_MK_INT, 1, 0, 0),
   M(correctionParams_projectors_LeftQ, "correction_projectors_LeftQ", correctionParams.projectors.LeftQ, PA_MK_INT, 1, 0, 0),
   M(correctionParams_projectors_LeftX, "correction_projectors_LeftX", correctionParams.projectors.LeftX, PA_MK_INT, 1, 0, 0),
   M(correctionParams_projectors_RightQ, "correction_projectors_RightQ", correctionParams.projectors.RightQ, PA_MK_INT, 1, 0, 0),
   M(correctionParams_projectors_RightX, "correction_projectors_RightX", correctionParams.projectors.RightX, PA_MK_INT, 1, 0, 0),
   M(correctionParams_projectors_SkewQ, "correction_projectors_SkewQ", correctionParams.projectors.SkewQ, PA_MK_INT, 1, 0, 0),
   M(correctionParams_projectors_SkewX, "correction_projectors_SkewX", correctionParams.projectors.SkewX, PA_MK_INT, 1, 0, 0),
   M(correctionParams_convTest, "correction_convTest", correctionParams.convTest, PA_MK_ENUM, 1, 0, PA_EN_CONVTEST),
   M(correctionParams_relTolBase, "correction_relTolBase", correctionParams.relTolBase, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_numOuterIterations, "stats_numOuterIterations", stats.numOuterIterations, PA_MK_LONG, 1, 0, 0),
   M(stats_numRestarts, "stats_numRestarts", stats.numRestarts, PA_MK_LONG, 1, 0, 0),
   M(stats_numMatvecs, "stats_numMatvecs", stats.numMatvecs, PA_MK_LONG, 1, 0, 0),
   M(stats_numPreconds, "stats_numPreconds", stats.numPreconds, PA_MK_LONG, 1, 0, 0),
   M(stats_numGlobalSum, "stats_numGlobalSum", stats.numGlobalSum, PA_MK_LONG, 1, PA_MF_NO_SET, 0),
   M(stats_volumeGlobalSum, "stats_volumeGlobalSum", stats.volumeGlobalSum, PA_MK_LONG, 1, 0, 0),
   M(stats_numBroadcast, "stats_numBroadcast", stats.numBroadcast, PA_MK_LONG, 1, PA_MF_NO_SET, 0),
   M(stats_volumeBroadcast, "stats_volumeBroadcast", stats.volumeBroadcast, PA_MK_LONG, 1, 0, 0),
   M(stats_flopsDense, "stats_flopsDense", stats.flopsDense, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_numOrthoInnerProds, "stats_numOrthoInnerProds", stats.numOrthoInnerProds, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_elapsedTime, "stats_elapsedTime", stats.elapsedTime, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_timeMatvec, "stats_timeMatvec", stats.timeMatvec, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_timePrecond, "stats_timePrecond", stats.timePrecond, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_timeOrtho, "stats_timeOrtho", stats.timeOrtho, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_timeGlobalSum, "stats_timeGlobalSum", stats.timeGlobalSum, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_timeBroadcast, "stats_timeBroadcast", stats.timeBroadcast, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_timeDense, "stats_timeDense", stats.timeDense, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_estimateMinEVal, "stats_estimateMinEVal", stats.estimateMinEVal, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_estimateMaxEVal, "stats_estimateMaxEVal", stats.estimateMaxEVal, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_estimateLargestSVal, "stats_estimateLargestSVal", stats.estimateLargestSVal, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_estimateBNorm, "stats_estimateBNorm", stats.estimateBNorm, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_estimateInvBNorm, "stats_estimateInvBNorm", stats.estimateInvBNorm, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_maxConvTol, "stats_maxConvTol", stats.maxConvTol, PA_MK_DOUBLE, 1, 0, 0),
   M(stats_lockingIssue, "stats_lockingIssue", stats.lockingIssue, PA_MK_LONG, 1, 0, 0),
   M(convTestFun, "convTestFun", convTestFun, PA_MK_POINTER, 1, 0, 0),
   M(convTestFun_type, "convTestFun_type", convTestFun_type, PA_MK_ENUM, 1, 0, 0),
   M(convtest, "convtest", convtest, PA_MK_POINTER, 1, 0, 0),
   M(ldevecs, "ldevecs", ldevecs, PA_MK_LONG, 1, 0, 0),
   M(ldOPs, "ldOPs", ldOPs, PA_MK_LONG, 1, 0, 0),
   M(monitorFun, "monitorFun", monitorFun, PA_MK_POINTER, 1, 0, 0),
   M(monitorFun_type, "monitorFun_type", monitorFun_type, PA_MK_ENUM, 1, 0, 0),
   M(monitor, "monitor", monitor, PA_MK_POINTER, 1, 0, 0),
   M(queue, "queue", queue, PA_MK_POINTER, 1, 0, 0),
   M(profile, "profile", profile, PA_MK_STRING, 1, 0, 0),
};
#undef M
#undef AT
#define EIGS_ROWS ((int)(sizeof(eigs_members) / sizeof(eigs_members[0])))

#define K(name, en) {#name, (int)name, en, 0}
#define K_SILENT(name, en) {#name, (int)name, en, 1}
static const pa_constant eigs_constants[] = {
   K(PRIMME_DEFAULT_METHOD, PA_EN_METHOD), K(PRIMME_DYNAMIC, PA_EN_METHOD), K(PRIMME_DEFAULT_MIN_TIME, PA_EN_METHOD),
   K(PRIMME_DEFAULT_MIN_MATVECS, PA_EN_METHOD), K(PRIMME_Arnoldi, PA_EN_METHOD), K(PRIMME_GD, PA_EN_METHOD),
   K(PRIMME_GD_plusK, PA_EN_METHOD), K(PRIMME_GD_Olsen_plusK, PA_EN_METHOD), K(PRIMME_JD_Olsen_plusK, PA_EN_METHOD),
   K(PRIMME_RQI, PA_EN_METHOD), K(PRIMME_JDQR, PA_EN_METHOD), K(PRIMME_JDQMR, PA_EN_METHOD), K(PRIMME_JDQMR_ETol, PA_EN_METHOD),
   K(PRIMME_STEEPEST_DESCENT, PA_EN_METHOD), K(PRIMME_LOBPCG_OrthoBasis, PA_EN_METHOD),
   K(PRIMME_LOBPCG_OrthoBasis_Window, PA_EN_METHOD),
   K(primme_smallest, PA_EN_TARGET), K(primme_largest, PA_EN_TARGET), K(primme_closest_geq, PA_EN_TARGET),
   K(primme_closest_leq, PA_EN_TARGET), K(primme_closest_abs, PA_EN_TARGET), K(primme_largest_abs, PA_EN_TARGET),
   K(primme_proj_default, PA_EN_PROJECTION), K(primme_proj_RR, PA_EN_PROJECTION), K(primme_proj_harmonic, PA_EN_PROJECTION),
   K(primme_proj_refined, PA_EN_PROJECTION),
   K(primme_init_default, PA_EN_INIT), K(primme_init_krylov, PA_EN_INIT), K(primme_init_random, PA_EN_INIT),
   K(primme_init_user, PA_EN_INIT),
   K(primme_full_LTolerance, PA_EN_CONVTEST), K(primme_decreasing_LTolerance, PA_EN_CONVTEST),
   K(primme_adaptive_ETolerance, PA_EN_CONVTEST), K(primme_adaptive, PA_EN_CONVTEST),
   K(primme_event_outer_iteration, PA_EN_EVENT), K(primme_event_inner_iteration, PA_EN_EVENT), K(primme_event_restart, PA_EN_EVENT),
   K(primme_event_reset, PA_EN_EVENT), K(primme_event_converged, PA_EN_EVENT), K(primme_event_locked, PA_EN_EVENT),
   K(primme_event_message, PA_EN_EVENT), K(primme_event_profile, PA_EN_EVENT),
   K_SILENT(primme_orth_default, PA_EN_ORTH), K(primme_orth_implicit_I, PA_EN_ORTH), K(primme_orth_explicit_I, PA_EN_ORTH),
   K_SILENT(primme_op_default, PA_EN_OP), K(primme_op_half, PA_EN_OP), K(primme_op_float, PA_EN_OP), K(primme_op_double, PA_EN_OP),
   K(primme_op_quad, PA_EN_OP), K_SILENT(primme_op_int, PA_EN_OP),
};
#define EIGS_CONSTANTS ((int)(sizeof(eigs_constants) / sizeof(eigs_constants[0])))

#define RULE "// ---------------------------------------------------\n"
#define L(style, label, aux) {style, PRIMME_##label, aux, NULL}
#define TEXT(t) {PA_DS_TEXT, 0, 0, t}
static const pa_display_line eigs_listing[] = {
   L(PA_DS_INT, n, 0), L(PA_DS_INT, nLocal, 0), L(PA_DS_INT, numProcs, 0), L(PA_DS_INT, procID, 0),
   TEXT("\n// Output and reporting\n"),
   L(PA_DS_INT, printLevel, 0),
   TEXT("\n// Solver parameters\n"),
   L(PA_DS_INT, numEvals, 0), L(PA_DS_E, aNorm, 0), L(PA_DS_E, BNorm, 0), L(PA_DS_E, invBNorm, 0), L(PA_DS_E, eps, 0),
   L(PA_DS_INT, maxBasisSize, 0), L(PA_DS_INT, minRestartSize, 0), L(PA_DS_INT, maxBlockSize, 0),
   L(PA_DS_INT, maxOuterIterations, 0), L(PA_DS_INT, maxMatvecs, 0),
   L(PA_DS_ENUM, target, PA_EN_TARGET), L(PA_DS_ENUM, projectionParams_projection, PA_EN_PROJECTION),
   L(PA_DS_ENUM, initBasisMode, PA_EN_INIT),
   L(PA_DS_INT, numTargetShifts, 0), L(PA_DS_SHIFTS, targetShifts, PRIMME_numTargetShifts),
   L(PA_DS_INT, dynamicMethodSwitch, 0), L(PA_DS_INT, locking, 0), L(PA_DS_INT, initSize, 0), L(PA_DS_INT, numOrthoConst, 0),
   L(PA_DS_INT, ldevecs, 0), L(PA_DS_INT, ldOPs, 0), L(PA_DS_SEED, iseed, 0),
   L(PA_DS_ENUM, orth, PA_EN_ORTH), L(PA_DS_ENUM, internalPrecision, PA_EN_OP),
   L(PA_DS_INT, restartingParams_maxPrevRetain, 0),
   TEXT("\n// Correction parameters\n"),
   L(PA_DS_INT, correctionParams_precondition, 0), L(PA_DS_INT, correctionParams_robustShifts, 0),
   L(PA_DS_INT, correctionParams_maxInnerIterations, 0), L(PA_DS_G, correctionParams_relTolBase, 0),
   L(PA_DS_ENUM, correctionParams_convTest, PA_EN_CONVTEST),
   TEXT("\n// projectors for JD cor.eq.\n"),
   L(PA_DS_INT, correctionParams_projectors_LeftQ, 0), L(PA_DS_INT, correctionParams_projectors_LeftX, 0),
   L(PA_DS_INT, correctionParams_projectors_RightQ, 0), L(PA_DS_INT, correctionParams_projectors_SkewQ, 0),
   L(PA_DS_INT, correctionParams_projectors_RightX, 0), L(PA_DS_INT, correctionParams_projectors_SkewX, 0),
   TEXT(RULE),
};

void pa_display_eigs(FILE *out, const char *prefix, primme_params *primme) {
   pa_display(out, prefix, eigs_members, EIGS_ROWS, primme, eigs_listing, (int)(sizeof(eigs_listing) / sizeof(eigs_listing[0])),
         eigs_constants, EIGS_CONSTANTS);
}

void primme_display_params(primme_params primme) {
   fputs(RULE "//                 primme configuration               \n" RULE, primme.outputFile);
   pa_display_eigs(primme.outputFile, "primme", &primme);
   fflush(primme.outputFile);
}

int primme_get_member(primme_params *primme, primme_params_label label, void *value) {
   return pa_member_get(eigs_members, EIGS_ROWS, primme, (int)label, value);
}

int primme_set_member(primme_params *primme, primme_params_label label, void *value) {
   return pa_member_set(eigs_members, EIGS_ROWS, primme, (int)label, value);
}

int primme_member_info(primme_params_label *label, const char **label_name, primme_type *type, int *arity) {
   int l = label ? (int)*label : 0;
   const int rc = pa_member_info(eigs_members, EIGS_ROWS, label ? &l : NULL, label_name, type, arity);
   if (label) *label = (primme_params_label)l;
   return rc;
}

int primme_constant_info(const char *label_name, int *value) {
   return pa_constant_info(eigs_constants, EIGS_CONSTANTS, label_name, value);
}

int primme_enum_member_info(primme_params_label label, int *value, const char **value_name) {
   return pa_enum_member_info(eigs_members, EIGS_ROWS, eigs_constants, EIGS_CONSTANTS, (int)label, value, value_name);
}
