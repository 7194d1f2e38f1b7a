/* amg_internal.h — the host stages of the algebraic multigrid set-up (csr_tools.c) that the device set-up of a hierarchy
 * (primme_amd_amg_hierarchy_create in amd_operator.hip) runs level by level: the aggregation always, the transfer matrices and
 * the triple product when a level falls back to the host.  Not part of the C ABI; documented at their definitions. */
#ifndef PRIMME_AMD_AMG_INTERNAL_H
#define PRIMME_AMD_AMG_INTERNAL_H
#include "primme_amd_io.h"
#ifdef __cplusplus
extern "C" {
#endif
int pa_amg_level0(int64_t n, const int32_t *rowptr, const int32_t *colind, const void *values, size_t elem_size, double shift,
      primme_amd_amg_level *L, double *dg);
int pa_amg_level_finish(primme_amd_amg_level *L, double *dg);
int64_t pa_amg_aggregate(const primme_amd_amg_level *L, const double *dg, double theta, int32_t *agg, int32_t *tmp);
int pa_amg_level_aggregate(primme_amd_amg_level *L, const double *dg, double theta, int32_t *tmp);
int pa_amg_prolongation(const primme_amd_amg_level *F, double omega, primme_amd_amg_transfer *X);
int pa_amg_galerkin_general(const primme_amd_amg_level *F, const primme_amd_amg_transfer *X, primme_amd_amg_level *Cl);
#ifdef __cplusplus
}
#endif
#endif
