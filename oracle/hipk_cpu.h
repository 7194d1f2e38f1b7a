/* oracle/hipk_cpu.h — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * What the files of the plain-C kernel layer (hipk_cpu.c, hipk_cpu_complex.c, hostcheck_glue.c) share among
 * themselves, and the entry points that only the tests call (through ctypes), declared once so that the build's
 * -Werror=missing-prototypes holds every definition against a prototype.  The C ABI of the device layer itself is
 * include/primme_amd_kernels.h; the product's internal names these files stand in for are in
 * primme_amd/csrc/eigs_internal.h.
 */
#ifndef ORACLE_HIPK_CPU_H
#define ORACLE_HIPK_CPU_H

#include <stddef.h>
#include <stdint.h>
#include "primme_amd_kernels.h"
#include "primme_amd_comm.h"

/* ---- hipk_cpu.c */
/* launch counters of the plain-C layer (tests assert the solver's launch structure) */
void hipk_cpu_counts(long *out, int reset);
/* keeps the zero-copy contract (results mirrored into pinned memory) on the host build */
void hipk_cpu_mirror(const double *out, size_t cnt);
/* installed by the stand-in communicator of hostcheck_glue.c: the results of a reduction pass through it before they are mirrored */
extern void (*hipk_cpu_xr_hook)(double *out, size_t cnt);

/* ---- hipk_cpu_complex.c: the complex instantiation, hipk_cpu.c dispatches here */
int hipk_z_panel_dots(hipk_dtype dt, int64_t m, const hipk_seg *segs, int nseg, const void *X, int64_t ldX, int nx, double *out, int ldout);
int hipk_z_panel_project_to(hipk_dtype dt, int64_t m, const hipk_seg *segs, int nseg, const double *coef, int ldcoef, const void *X, int64_t ldX, void *Xout, int64_t ldXout, int nx, double *nrm2);
int hipk_z_panel_project_mul(hipk_dtype dt, int64_t m, const hipk_seg *segs, int nseg, const double *coef, int ldcoef, const double *M, void *X, int64_t ldX, int nx);
int hipk_z_ritz_update(hipk_dtype dt, int64_t m, const void *V, const void *W, int64_t ld, int k, const double *h, int ldh, const double *theta, const hipk_job *jobs, int njobs, double *nrm2);
int hipk_z_scale_cols(hipk_dtype dt, int64_t m, void *X, int64_t ldX, int nx, const double *a);
int hipk_z_axpy_cols(hipk_dtype dt, int64_t m, const double *a, const void *X, int64_t ldX, void *Y, int64_t ldY, int nx);
int hipk_z_xpay_cols(hipk_dtype dt, int64_t m, const double *a, const void *X, int64_t ldX, void *Y, int64_t ldY, int nx);
int hipk_z_col_norms2(hipk_dtype dt, int64_t m, const void *X, int64_t ldX, int nx, double *out);
int hipk_z_residual_cols(hipk_dtype dt, int64_t m, const void *X, int64_t ldX, void *Wr, int64_t ldW, int nx, const double *theta, double *nrm2);
int hipk_z_pair_dots(hipk_dtype dt, int64_t m, const void *X, int64_t ldX, const void *Y, int64_t ldY, int nx, double *out);
int hipk_z_csr_matvec(hipk_dtype dt, int64_t nrows, const int32_t *rp, const int32_t *ci, const void *val, int64_t x0, int64_t xlen, int64_t halo_lo, const void *xlo, int64_t ld_lo, const void *xhi, int64_t ld_hi, const void *x, int64_t ldx, void *y, int64_t ldy, int ncols, const double *shift);
int hipk_z_jacobi_apply(hipk_dtype dt, int64_t m, const void *diag, const double *shift, double min_den, const void *x, int64_t ldx, void *y, int64_t ldy, int ncols);

/* ---- hostcheck_glue.c: the stand-in communicator of the tests (the all-reduce is a callback of the test) */
typedef void (*hostcheck_allreduce_fn)(double *buf, int count);
int primme_amd_hostcheck_comm_create(primme_amd_comm **out, hostcheck_allreduce_fn cb, int rank, int size);
long primme_amd_hostcheck_comm_calls(const primme_amd_comm *c);
/* switch the stand-in of the fused cross-rank second stage on for this communicator */
int primme_amd_hostcheck_comm_set_xr(primme_amd_comm *c, int on);
long primme_amd_hostcheck_comm_xr_calls(const primme_amd_comm *c);

#endif
