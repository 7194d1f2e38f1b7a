/* amd_operator.hip — the ready-made matrixMatvec / applyPreconditioner callbacks
 * (include/primme_amd.h) over a device sparse operator, with the halo exchange of
 * the row-partitioned case.  Replaces the per-application callback code of
 * reference examples/ex_eigs_dhipblas.c:239-264 and examples/ex_eigs_mpi.c:150-207.
 */
#include "hipk_internal.h"
#include "primme_amd.h"
#include "primme_amd_comm.h"
#include "comm_internal.h"
#include "eigs_internal.h"   /* primme_amd_svds_operator_is_local */
#include "primme_amd_io.h"     /* primme_amd_amg_plan */
#include "amg_internal.h"      /* the host stages of the hierarchy's device set-up */
#include <time.h>

/* aggregation AMG preconditioner (primme_amd_amg_precond): the hierarchy on the device, nlev = 0 until configured.  Level l
   has n rows, nc aggregates (0 on the last level), the operator M (level 0: NULL, the operator's own matrix serves with the
   shift folded into the product), dinv = 1 / diag(M_l), the spectral bound rho and the aggregate maps; ld elements per scratch
   column (16-byte columns).  G: the dense inverse of the last level when it has at most PRIMME_AMD_AMG_DENSE_ROWS rows.
   buf: ONE allocation of cols columns per panel, level 0 an iterate and the product, every other level the right-hand side,
   two iterates and the product.  Smoothed aggregation (set_amg_smoothed): P_l (n rows) and R_l = P_l' (nc rows) in CSR with
   double values, NULL for plain aggregation.
   The levels live in a reference-counted HIERARCHY (primme_amd_amg_hierarchy_create) that several operators over
   the same matrix may share: the handle its creator holds counts one, every operator it is attached to one.  Beside the
   operator M[0] (double panels) / M[1] (float panels) of a level >= 1, made when the hierarchy is first attached to an operator
   of that type, it keeps the level's CSR arrays in double (mrp, mci, mva): what the device set-up builds, what the operators are
   made from and what primme_amd_amg_hierarchy_download reads.  An operator's own state is the attachment: the smoother's
   parameters, the operator type and the scratch panels */
struct amg_level_dev {
   int64_t n, nc, ld, nnz, pnnz;
   double rho;
   hipk_csr *M[2];
   int32_t *mrp, *mci;
   double *mva;
   double *dinv;
   int32_t *agg, *aggptr, *aggrows;
   int32_t *prp, *pci, *rrp, *rci;
   double *pva, *rva;
};
#define AMG_NSTAGES 6                       /* aggregation (host), P, R, triple product, finish, download of M_{l+1} */
struct primme_amd_amg_hierarchy {
   int refs, nlev, smoothed, fallback, own_ctx;
   int priv;                                /* 1 + the operator type (0 double, 1 float) of the one operator a private hierarchy of
                                               set_amg[_smoothed] serves: its level operators are made at once, no CSR arrays kept */
   int64_t max_entries;                     /* the entry limit of the device stages */
   long attached;
   hipk_ctx *ctx;
   double shift, theta, omega;
   int64_t n0, nnz0;
   amg_level_dev lv[PRIMME_AMD_AMG_MAXLEVELS];
   double *G;
   double setup_seconds, device_seconds, stage[PRIMME_AMD_AMG_MAXLEVELS][AMG_NSTAGES];
};
struct amg_state {
   primme_amd_amg_hierarchy *h;             /* NULL until configured */
   int dti, nu, cs, cols;
   double over;
   void *buf;
};

struct primme_amd_operator {
   hipk_csr *A;
   primme_amd_comm *comm;
   int mode;                 /* 0 local, 1 neighbour halo, 2 all-gather */
   int64_t lo, hi;           /* rows needed from below / above */
   int64_t send_lo, send_hi; /* rows the neighbours need from me */
   int64_t max_side;         /* the largest halo of any rank (sizes the peer-to-peer landing zones) */
   void *buf_lo, *buf_hi;    /* device halo buffers (grown on demand) */
   size_t cap_lo, cap_hi;
   void *xfull;              /* all-gather buffer */
   size_t cap_full;
   int64_t row0, nrows, n;
   int jacobi_fixed;         /* 1: K = diag(A) - jacobi_shift, 0: per-vector shifts of the solver */
   double jacobi_shift;
   int ldscale;              /* 2 when A is the real-equivalent form of a Hermitian matrix and the
                                callbacks are handed leading dimensions in complex elements */
   /* Chebyshev polynomial preconditioner (primme_amd_chebyshev_precond): steps = 0 until configured */
   int cheb_steps, cheb_fixed, cheb_unfused, cheb_fused_all;
   double cheb_lo, cheb_hi, cheb_shift;
   void *cheb_y, *cheb_w;    /* device scratch: the two iterates that are not the caller's (2 x cheb_cols columns) and the
                                operator product of the generic path (cheb_cols columns), cheb_ld elements apart */
   int cheb_cols, cheb_wcols;
   int64_t cheb_ld;
   /* geometric multigrid preconditioner (primme_amd_multigrid_precond): mg_nlev = 0 until configured.  Level l has the grid
      mg_n[l] with weights mg_w[l], mg_ld[l] elements per scratch column (16-byte columns) and, in ONE allocation of mg_cols
      columns per panel, a temporary (level 0; the other iterate is the caller's y) or the right-hand side and two iterates */
   int mg_nlev, mg_nu, mg_cs, mg_cols;
   double mg_scale, mg_shift;
   int mg_n[PRIMME_AMD_MG_MAXLEVELS][3];
   double mg_w[PRIMME_AMD_MG_MAXLEVELS][3];
   int64_t mg_ld[PRIMME_AMD_MG_MAXLEVELS];
   void *mg_buf;
   amg_state amg;
};
static void amg_release(amg_state *s);

static size_t op_elem(hipk_dtype dt) { return dt == HIPK_F64 ? 8 : dt == HIPK_F32 ? 4 : dt == HIPK_C64 ? 16 : 8; }

extern "C" int primme_amd_operator_create(primme_amd_operator **out, hipk_csr *A, primme_amd_comm *comm) {
   primme_amd_operator *op = (primme_amd_operator *)calloc(1, sizeof(*op));
   if (!op) return -2;
   op->A = A; op->comm = comm; op->ldscale = 1;
   op->lo = hipk_csr_halo_lo(A); op->hi = hipk_csr_halo_hi(A);
   op->nrows = hipk_csr_nrows(A);
   if ((op->lo > 0 || op->hi > 0) && !comm) {
      fprintf(stderr, "primme_amd: operator references rows outside the local slab but no communicator was given\n");
      free(op);
      return -1;
   }
   if (comm && primme_amd_comm_size(comm) > 1) {
      const int P = primme_amd_comm_size(comm), r = primme_amd_comm_rank(comm);
      int64_t mine[3] = {op->lo, op->hi, op->nrows};
      int64_t *all = (int64_t *)malloc((size_t)P * 3 * sizeof(int64_t));
      if (primme_amd_comm_allgather_i64(comm, mine, 3, all)) { free(all); free(op); return -43; }
      int neighbour_ok = 1, any = 0, equal = 1;
      for (int q = 0; q < P; q++) {
         if (all[3 * q] > 0 || all[3 * q + 1] > 0) any = 1;
         if (all[3 * q] > op->max_side) op->max_side = all[3 * q];
         if (all[3 * q + 1] > op->max_side) op->max_side = all[3 * q + 1];
         if (q > 0 && all[3 * q] > all[3 * (q - 1) + 2]) neighbour_ok = 0;     /* needs more than rank q-1 owns */
         if (q < P - 1 && all[3 * q + 1] > all[3 * (q + 1) + 2]) neighbour_ok = 0;
         if (all[3 * q + 2] != all[2]) equal = 0;
      }
      if (!any) op->mode = 0;
      else if (neighbour_ok) {
         op->mode = 1;
         op->send_hi = (r < P - 1) ? all[3 * (r + 1)] : 0;     /* what rank r+1 needs from below = my last rows */
         op->send_lo = (r > 0) ? all[3 * (r - 1) + 1] : 0;     /* what rank r-1 needs from above = my first rows */
      } else {
         if (!equal) {
            fprintf(stderr, "primme_amd: all-gather matvec needs equal slabs per rank\n");
            free(all); free(op);
            return -1;
         }
         op->mode = 2;
      }
      int64_t r0 = 0, n = 0;
      for (int q = 0; q < P; q++) { if (q < r) r0 += all[3 * q + 2]; n += all[3 * q + 2]; }
      op->row0 = r0; op->n = n;
      free(all);
   }
   *out = op;
   return 0;
}

extern "C" int primme_amd_operator_destroy(primme_amd_operator *op) {
   if (!op) return 0;
   if (op->buf_lo) (void)hipFree(op->buf_lo);
   if (op->buf_hi) (void)hipFree(op->buf_hi);
   if (op->xfull) (void)hipFree(op->xfull);
   if (op->cheb_y) (void)hipFree(op->cheb_y);
   if (op->cheb_w) (void)hipFree(op->cheb_w);
   if (op->mg_buf) (void)hipFree(op->mg_buf);
   amg_release(&op->amg);
   free(op);
   return 0;
}

extern "C" hipk_csr *primme_amd_operator_matrix(primme_amd_operator *op) { return op->A; }

static int grow(void **buf, size_t *cap, size_t need) {
   if (need <= *cap) return 0;
   if (*buf) HIPK_CHECK(hipFree(*buf));
   HIPK_CHECK(hipMalloc(buf, need));
   *cap = need;
   return 0;
}

extern "C" int primme_amd_operator_apply(primme_amd_operator *op, void *hip_stream, const void *x,
      int64_t ldx, void *y, int64_t ldy, int ncols) {
   const size_t es = op_elem(hipk_csr_dtype(op->A));
   if (op->mode == 1) {
      if (grow(&op->buf_lo, &op->cap_lo, (size_t)(op->lo > 0 ? op->lo : 1) * ncols * es)) return -2;
      if (grow(&op->buf_hi, &op->cap_hi, (size_t)(op->hi > 0 ? op->hi : 1) * ncols * es)) return -2;
      void *zl = NULL, *zh = NULL;
      int rc = pa_comm_halo_auto(op->comm, hip_stream, x, ldx, op->nrows, ncols, es, op->send_lo,
            op->send_hi, op->buf_lo, op->lo, op->buf_hi, op->hi, op->max_side, &zl, &zh);
      if (rc) return rc;
      hipk_csr_set_halo(op->A, zl, zh);
      return hipk_csr_matvec(op->A, hip_stream, x, ldx, y, ldy, ncols);
   } else if (op->mode == 2) {
      /* unstructured columns: gather the whole block [n x ncols] in ONE grouped exchange (a column per
       * all-gather inside an RCCL group = one launch), then one SpMM; lo = everything below my slab,
       * hi = everything above, both addressed inside the gathered block with column stride n */
      if (grow(&op->xfull, &op->cap_full, (size_t)op->n * ncols * es)) return -2;
      int rc = primme_amd_comm_allgather_cols(op->comm, hip_stream, x, ldx, op->xfull, op->n, (size_t)op->nrows * es, es, ncols);
      if (rc) return rc;
      hipk_csr_set_halo_ld(op->A, (const char *)op->xfull + (size_t)(op->row0 - op->lo) * es, op->n,
            (const char *)op->xfull + (size_t)(op->row0 + op->nrows) * es, op->n);
      return hipk_csr_matvec(op->A, hip_stream, x, ldx, y, ldy, ncols);
   }
   return hipk_csr_matvec(op->A, hip_stream, x, ldx, y, ldy, ncols);
}

/* One-synchronisation GD iteration (eigs_conv.c): y = A (a x), xout = a x, dot_dev[0] = xout' y with
 * a = 1/sqrt(norm2_dev[0]) in ONE launch (hipk_csr_matvec_scaled), halo exchange included.  Only for the
 * solver's own use with this ready-made operator: a user matvec callback is a black box and gets the
 * separate normalisation / operator / inner-product launches instead. */
extern "C" int primme_amd_operator_can_fuse(const primme_amd_operator *op) {
   /* every precondition of hipk_csr_matvec_scaled, so that an eligible tail cannot fail with "not applicable":
    * a CSR matrix whose input entries are its own row slab, and halo data this operator knows how to fetch */
   if (!op || op->ldscale != 1 || !hipk_csr_fusable(op->A)) return 0;
   if (op->mode == 0 && (hipk_csr_halo_lo(op->A) > 0 || hipk_csr_halo_hi(op->A) > 0)) return 0;
   return 1;
}
extern "C" int primme_amd_operator_apply_scaled(primme_amd_operator *op, hipk_ctx *ctx, const void *x,
      const double *norm2_dev, void *xout, void *y, double *dot_dev) {
   if (!primme_amd_operator_can_fuse(op) || !ctx) return -1;
   void *hip_stream = hipk_ctx_stream(ctx);
   const size_t es = op_elem(hipk_csr_dtype(op->A));
   if (op->mode == 1) {
      if (grow(&op->buf_lo, &op->cap_lo, (size_t)(op->lo > 0 ? op->lo : 1) * es)) return -2;
      if (grow(&op->buf_hi, &op->cap_hi, (size_t)(op->hi > 0 ? op->hi : 1) * es)) return -2;
      void *zl = NULL, *zh = NULL;
      int rc = pa_comm_halo_auto(op->comm, hip_stream, x, op->nrows, op->nrows, 1, es, op->send_lo,
            op->send_hi, op->buf_lo, op->lo, op->buf_hi, op->hi, op->max_side, &zl, &zh);
      if (rc) return rc;
      hipk_csr_set_halo(op->A, zl, zh);
   } else if (op->mode == 2) {
      if (grow(&op->xfull, &op->cap_full, (size_t)op->n * es)) return -2;
      int rc = primme_amd_comm_allgather(op->comm, hip_stream, x, op->xfull, (size_t)op->nrows * es);
      if (rc) return rc;
      hipk_csr_set_halo(op->A, (const char *)op->xfull + (size_t)(op->row0 - op->lo) * es,
            (const char *)op->xfull + (size_t)(op->row0 + op->nrows) * es);
   }
   return hipk_csr_matvec_scaled(op->A, ctx, x, norm2_dev, xout, y, dot_dev);
}

extern "C" int primme_amd_operator_apply_shifted(primme_amd_operator *op, void *hip_stream, const void *x, int64_t ldx,
      void *y, int64_t ldy, int ncols, const double *shifts_host) {
   if (!op || op->mode != 0 || op->ldscale != 1) return 1;
   return hipk_csr_matvec_shifted(op->A, hip_stream, x, ldx, y, ldy, ncols, shifts_host);
}
extern "C" int primme_amd_operator_jacobi_data(primme_amd_operator *op, const void **diag, int *fixed, double *shift) {
   if (!op || op->ldscale != 1) return 1;
   *diag = hipk_csr_diag(op->A); *fixed = op->jacobi_fixed; *shift = op->jacobi_shift;
   return 0;
}

/* ---- the callbacks ---------------------------------------------------------- */
extern "C" void primme_amd_mass_matvec(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy, int *blockSize,
      struct primme_params *primme, int *ierr) {
   primme_amd_operator *op = (primme_amd_operator *)primme->massMatrix;
   void *stream = primme->queue ? (void *)*(hipStream_t *)primme->queue : NULL;
   *ierr = op ? primme_amd_operator_apply(op, stream, x, *ldx * op->ldscale, y, *ldy * op->ldscale, *blockSize) : 1;
}
extern "C" void primme_amd_matvec(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy, int *blockSize,
      struct primme_params *primme, int *ierr) {
   primme_amd_operator *op = (primme_amd_operator *)primme->matrix;
   void *stream = primme->queue ? (void *)*(hipStream_t *)primme->queue : NULL;
   *ierr = op ? primme_amd_operator_apply(op, stream, x, *ldx * op->ldscale, y, *ldy * op->ldscale, *blockSize) : 1;
}

extern "C" void primme_amd_jacobi_precond(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy,
      int *blockSize, struct primme_params *primme, int *ierr) {
   primme_amd_operator *op = (primme_amd_operator *)primme->preconditioner;
   void *stream = primme->queue ? (void *)*(hipStream_t *)primme->queue : NULL;
   if (!op) { *ierr = 1; return; }
   const hipk_dtype dt = hipk_csr_dtype(op->A);
   const size_t es = op_elem(dt);
   const int64_t lx = *ldx * op->ldscale, ly = *ldy * op->ldscale;
   *ierr = 0;
   for (int c0 = 0; c0 < *blockSize && !*ierr; c0 += 64) {
      const int n = *blockSize - c0 < 64 ? *blockSize - c0 : 64;
      double fixed[64];
      for (int c = 0; c < n; c++) fixed[c] = op->jacobi_shift;
      *ierr = hipk_jacobi_apply(stream, dt, hipk_csr_nrows(op->A), hipk_csr_diag(op->A),
            op->jacobi_fixed ? fixed : primme->ShiftsForPreconditioner + c0,
            1e-14 * (primme->aNorm >= 0.0 ? primme->aNorm : 1.0), (const char *)x + (size_t)c0 * lx * es, lx,
            (char *)y + (size_t)c0 * ly * es, ly, n);
   }
}

/* ---- Chebyshev polynomial preconditioner K^-1 = p(A) (kernels in hipk_cheb.hip) -----------------------
 * y = p(A) x is the d-th iterate of Chebyshev iteration for (A - sigma I) y = x from y_0 = 0 with the interval [lo, hi]:
 *    tb = (hi + lo)/2 - sigma, dl = (hi - lo)/2, s1 = tb/dl, rho_1 = 1/s1, y_1 = x/tb,
 *    rho_{k+1} = 1/(2 s1 - rho_k),  y_{k+1} = y_k + rho_{k+1} rho_k (y_k - y_{k-1}) + (2 rho_{k+1}/dl)(x - (A - sigma I) y_k),
 * d - 1 operator applications.  Written as the linear combination the kernels take, with a = rho_{k+1} rho_k, b = 2 rho_{k+1}/dl:
 *    y_{k+1} = (1 + a + b sigma) y_k - a y_{k-1} + b x - b A y_k.
 * y_1 is never stored: step 1 gathers from x itself (coefficients divided by tb), step 2 reads x for y_{k-1} the same way.
 * The iterates alternate between the two scratch panels, y_{k+1} over y_{k-1}; the last one goes to the caller's y. */
/* Widest block for which the fused step is the default, per operator form: where the kernel trace shows it not slower than
 * the operator product + cheb_update_kernel (profiles/cheb_step_kernels.md).  PRIMME_AMD_CHEB_FUSED=1 fuses at every width,
 * PRIMME_AMD_CHEB_UNFUSED=1 at none. */
#define CHEB_FUSE_PAT_MAXCOLS 8
#define CHEB_FUSE_CSR_MAXCOLS 0
static long g_cheb_applies, g_cheb_products, g_cheb_fused;
extern "C" void primme_amd_chebyshev_stats(long *applies, long *operator_products, long *fused_steps) {
   if (applies) *applies = g_cheb_applies;
   if (operator_products) *operator_products = g_cheb_products;
   if (fused_steps) *fused_steps = g_cheb_fused;
   g_cheb_applies = g_cheb_products = g_cheb_fused = 0;
}

extern "C" int primme_amd_operator_gershgorin(primme_amd_operator *op, double *lo, double *hi) {
   if (!op || !lo || !hi) return -1;
   double b[2];
   int rc = hipk_csr_gershgorin(op->A, NULL, b);
   if (rc) return rc;
   if (op->comm && primme_amd_comm_size(op->comm) > 1) {
      /* every rank's pair, as bit patterns; an empty slab's (+inf, -inf) is neutral for min / max */
      const int P = primme_amd_comm_size(op->comm);
      int64_t mine[2], *all = (int64_t *)malloc((size_t)2 * P * sizeof(int64_t));
      if (!all) return -2;
      memcpy(mine, b, sizeof(mine));
      rc = primme_amd_comm_allgather_i64(op->comm, mine, 2, all);
      for (int q = 0; q < P && !rc; q++) {
         double bq[2];
         memcpy(bq, all + 2 * q, sizeof(bq));
         if (bq[0] < b[0]) b[0] = bq[0];
         if (bq[1] > b[1]) b[1] = bq[1];
      }
      free(all);
      if (rc) return rc;
   }
   *lo = b[0]; *hi = b[1];
   return 0;
}

extern "C" int primme_amd_operator_set_chebyshev(primme_amd_operator *op, int steps, double lo, double hi, int fixed, double shift) {
   if (!op || steps < 1 || lo != lo) return -1;          /* lo = NaN: there is no sensible default for the lower end */
   if (hi != hi) {                                       /* hi = NaN: the Gershgorin upper bound (collective over the ranks) */
      double glo, ghi;
      if (primme_amd_operator_gershgorin(op, &glo, &ghi)) return -1;
      hi = ghi;
   }
   if (!(lo < hi)) return -1;
   if (fixed && (shift != shift || (shift > lo && shift < hi))) return -1;
   op->cheb_steps = steps; op->cheb_lo = lo; op->cheb_hi = hi; op->cheb_fixed = fixed != 0; op->cheb_shift = shift;
   /* A/B knob, read when the preconditioner is configured (once per solve through the Python driver) */
   const char *e = getenv("PRIMME_AMD_CHEB_UNFUSED");
   op->cheb_unfused = e && atoi(e) != 0;
   e = getenv("PRIMME_AMD_CHEB_FUSED");                  /* opt in to the fused step at every width (see CHEB_FUSE_*_MAXCOLS) */
   op->cheb_fused_all = e && atoi(e) != 0;
   return 0;
}

/* coefficients of step k (1 .. d-1) for one column; rho = rho_k on entry, rho_{k+1} on return */
static void cheb_step_coef(double tb, double dl, double sigma, int k, double *rho, hipk_cheb_coef *cf, int c) {
   const double s1 = tb / dl, rn = 1.0 / (2.0 * s1 - *rho), a = rn * *rho, b = 2.0 * rn / dl;
   const double cy = 1.0 + a + b * sigma;
   cf->cy[c] = k == 1 ? cy / tb : cy;          /* step 1: y_k is x / tb */
   cf->cp[c] = k == 1 ? 0.0 : (k == 2 ? -a / tb : -a);      /* step 2: y_{k-1} is x / tb */
   cf->cx[c] = b;
   cf->cw[c] = k == 1 ? -b / tb : -b;
   *rho = rn;
}

extern "C" void primme_amd_chebyshev_precond(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy,
      int *blockSize, struct primme_params *primme, int *ierr) {
   primme_amd_operator *op = (primme_amd_operator *)primme->preconditioner;
   void *stream = primme->queue ? (void *)*(hipStream_t *)primme->queue : NULL;
   if (!op || op->cheb_steps < 1) { *ierr = 1; return; }
   if (!op->cheb_fixed && primme->target != primme_smallest && primme->target != primme_largest) {
      if (primme->printLevel > 0 && primme->outputFile)
         fprintf(primme->outputFile, "primme_amd: the Chebyshev preconditioner follows the solver's shifts for the smallest / largest targets only (use a fixed shift)\n");
      *ierr = 1;
      return;
   }
   *ierr = 0;
   if (*blockSize <= 0) return;
   if (!stream) stream = hipk_ctx_stream(hipk_csr_ctx(op->A));
   const hipk_dtype dt = hipk_csr_dtype(op->A);
   const size_t es = op_elem(dt);
   const int64_t m = hipk_csr_nrows(op->A);
   const int64_t lx = *ldx * op->ldscale, ly = *ldy * op->ldscale;
   const int d = op->cheb_steps;
   const double lo = op->cheb_lo, hi = op->cheb_hi, dl = 0.5 * (hi - lo);
   /* scratch for the widest chunk seen; columns on 16-byte boundaries */
   const int want = *blockSize < HIPK_CHEB_MAXCOLS ? *blockSize : HIPK_CHEB_MAXCOLS;
   const int64_t ld = (m + 3) / 4 * 4 + 4;
   if (d > 1 && (want > op->cheb_cols || ld != op->cheb_ld)) {
      if (op->cheb_y) (void)hipFree(op->cheb_y);
      if (op->cheb_w) (void)hipFree(op->cheb_w);
      op->cheb_y = op->cheb_w = NULL; op->cheb_cols = op->cheb_wcols = 0;
      if (hipMalloc(&op->cheb_y, (size_t)ld * es * 2 * want) != hipSuccess) { *ierr = 1; return; }
      op->cheb_cols = want; op->cheb_ld = ld;
   }
   /* the fused step serves real single-rank CSR operators whose vectors are what the solver hands over */
   int fused_ok = !op->cheb_unfused && op->mode == 0 && op->ldscale == 1 && !(op->comm && primme_amd_comm_size(op->comm) > 1);
   const int fuse_maxcols = hipk_csr_format(op->A) == 2 ? CHEB_FUSE_PAT_MAXCOLS : CHEB_FUSE_CSR_MAXCOLS;
   char *P[2] = {(char *)op->cheb_y, (char *)op->cheb_y + (size_t)ld * es * op->cheb_cols};
   for (int c0 = 0; c0 < *blockSize && !*ierr; c0 += HIPK_CHEB_MAXCOLS) {
      const int nc = *blockSize - c0 < HIPK_CHEB_MAXCOLS ? *blockSize - c0 : HIPK_CHEB_MAXCOLS;
      const char *xc = (const char *)x + (size_t)c0 * lx * es;
      char *yc = (char *)y + (size_t)c0 * ly * es;
      double sig[HIPK_CHEB_MAXCOLS], tb[HIPK_CHEB_MAXCOLS], rho[HIPK_CHEB_MAXCOLS];
      hipk_cheb_coef cf;
      memset(&cf, 0, sizeof(cf));
      for (int c = 0; c < nc; c++) {
         double sg = op->cheb_shift;
         if (!op->cheb_fixed) {
            /* the solver's shift, kept outside the open interval: at the clamp s1 = +-1 and the recurrence stays finite */
            const int small = primme->target == primme_smallest;
            sg = primme->ShiftsForPreconditioner ? primme->ShiftsForPreconditioner[c0 + c] : (small ? lo : hi);
            if (small ? !(sg <= lo) : !(sg >= hi)) sg = small ? lo : hi;
         }
         sig[c] = sg; tb[c] = 0.5 * (hi + lo) - sg; rho[c] = dl / tb[c];
         cf.cx[c] = 1.0 / tb[c];
      }
      g_cheb_applies += nc;
      if (d == 1) {
         *ierr = hipk_cheb_update(stream, dt, m, nc, &cf, xc, lx, NULL, 0, NULL, 0, NULL, 0, yc, ly) ? 1 : 0;
         continue;
      }
      for (int k = 1; k < d && !*ierr; k++) {
         for (int c = 0; c < nc; c++) cheb_step_coef(tb[c], dl, sig[c], k, &rho[c], &cf, c);
         /* y_k: x (k = 1) or a scratch panel; y_{k-1}: none, x (k = 2) or the other panel; y_{k+1} over y_{k-1}, the last into y */
         const char *yk = k == 1 ? xc : P[k % 2], *yp = k == 1 ? NULL : (k == 2 ? xc : P[(k + 1) % 2]);
         const int64_t ldk = k == 1 ? lx : ld, ldp = k == 2 ? lx : ld;
         char *out = k == d - 1 ? yc : P[(k + 1) % 2];
         const int64_t ldo = k == d - 1 ? ly : ld;
         int rc = 1;
         if (fused_ok && (op->cheb_fused_all || nc <= fuse_maxcols)) {
            rc = hipk_csr_cheb_step(op->A, stream, nc, &cf, xc, lx, yk, ldk, yp, ldp, out, ldo);
            if (rc == 1) fused_ok = 0;            /* no fused form for this operator: the generic path from here on */
            else if (rc == 0) g_cheb_fused += nc;
         }
         if (rc == 1) {
            if (op->cheb_wcols < op->cheb_cols) {       /* the product's panel: only the generic path needs it */
               if (op->cheb_w) (void)hipFree(op->cheb_w);
               op->cheb_w = NULL; op->cheb_wcols = 0;
               if (hipMalloc(&op->cheb_w, (size_t)ld * es * op->cheb_cols) != hipSuccess) { *ierr = 1; return; }
               op->cheb_wcols = op->cheb_cols;
            }
            rc = primme_amd_operator_apply(op, stream, yk, ldk, op->cheb_w, ld, nc);
            if (!rc) rc = hipk_cheb_update(stream, dt, m, nc, &cf, xc, lx, op->cheb_w, ld, yk, ldk, yp, ldp, out, ldo);
         }
         g_cheb_products += nc;
         if (rc) *ierr = 1;
      }
   }
}

/* ---- geometric multigrid preconditioner for grid Laplacians (kernels in hipk_mg.hip) --------------------
 * y = K^-1 x: one symmetric V(nu, nu) cycle from zero for M = scale L + shift I on the grid given to set_multigrid,
 *    vcycle(l, b):  l == last: nu_c Chebyshev steps from zero over the exact spectrum of M_l
 *                   y = nu Chebyshev steps from zero;  y += P vcycle(l + 1, R (b - M_l y));  nu Chebyshev steps from y
 * with the smoother's interval [hi_l / (2 D_l), hi_l].  The post-smoother is the SAME iteration started at y (first step
 * y + (b - M y) / tb): with p the smoother's polynomial it returns y + p(M)(b - M y), which makes K symmetric, in nu passes
 * instead of a residual, nu - 1 steps and an update.  Every pass is one hipk_mg_stencil_step: a Chebyshev step (coefficients of
 * cheb_step_coef with sigma = -shift, the product's scaled by `scale`) or the residual.  Per level the iterates alternate
 * between two panels, y_{k+1} over y_{k-1}; which of the two a sequence starts in is chosen so that its last iterate lands
 * where the next stage expects it (level 0: in the caller's y). */
static long g_mg_applies, g_mg_launches;
extern "C" void primme_amd_multigrid_stats(long *applies, long *launches) {
   if (applies) *applies = g_mg_applies;
   if (launches) *launches = g_mg_launches;
   g_mg_applies = g_mg_launches = 0;
}

/* exact ends of the spectrum of M_l and D_l, the number of dimensions with more than one point */
static void mg_level_ends(const primme_amd_operator *op, int l, double *lo, double *hi, int *D) {
   double a = 0.0, b = 0.0;
   int nd = 0;
   for (int d = 0; d < 3; d++)
      if (op->mg_n[l][d] > 1) {
         const double c = cos(M_PI / (op->mg_n[l][d] + 1));
         a += op->mg_w[l][d] * (2.0 - 2.0 * c);
         b += op->mg_w[l][d] * (2.0 + 2.0 * c);
         nd++;
      }
   *lo = op->mg_scale * a + op->mg_shift; *hi = op->mg_scale * b + op->mg_shift; *D = nd;
}

extern "C" int primme_amd_operator_set_multigrid(primme_amd_operator *op, int nx, int ny, int nz, int smooth_steps, int coarse_steps,
      double scale, double shift) {
   if (!op) return -1;
   const hipk_dtype dt = hipk_csr_dtype(op->A);
   if (op->mode != 0 || (op->comm && primme_amd_comm_size(op->comm) > 1) || op->ldscale != 1 || (dt != HIPK_F64 && dt != HIPK_F32)) return -44;
   if (nx < 1 || ny < 1 || nz < 1 || smooth_steps < 1 || coarse_steps < 1 || !(scale > 0.0) || !(shift >= 0.0)) return -1;
   if ((int64_t)nx * ny > INT32_MAX || (int64_t)nx * ny * nz != hipk_csr_nrows(op->A)) return -1;
   primme_amd_operator cand = *op;                 /* the operator changes only when everything is in order */
   const int dims[3] = {nx, ny, nz};
   if (primme_amd_mg_plan(dims, &cand.mg_nlev, cand.mg_n, cand.mg_w)) return -1;
   cand.mg_nu = smooth_steps; cand.mg_cs = coarse_steps; cand.mg_scale = scale; cand.mg_shift = shift;
   double lo, hi;
   int D;
   mg_level_ends(&cand, cand.mg_nlev - 1, &lo, &hi, &D);
   if (!(lo > 0.0)) return -1;                     /* one grid point and no shift: M = 0 */
   for (int l = 0; l < cand.mg_nlev; l++) cand.mg_ld[l] = ((int64_t)cand.mg_n[l][0] * cand.mg_n[l][1] * cand.mg_n[l][2] + 3) / 4 * 4;
   if (op->mg_buf) (void)hipFree(op->mg_buf);      /* another grid: the scratch is laid out again at the next application */
   cand.mg_buf = NULL; cand.mg_cols = 0;
   *op = cand;
   return 0;
}

struct mg_run {
   primme_amd_operator *op;
   void *stream;
   hipk_dtype dt;
   size_t es;
   int nc;
   int rc;
};
static void mg_step(mg_run *r, int l, const hipk_cheb_coef *cf, const char *x, int64_t lx, const char *yk, int64_t ldk, const char *yp,
      int64_t ldp, char *out, int64_t ldo) {
   if (r->rc) return;
   r->rc = hipk_mg_stencil_step(r->stream, r->dt, r->op->mg_n[l], r->op->mg_w[l], r->nc, cf, x, lx, yk, ldk, yp, ldp, out, ldo);
   g_mg_launches++;
}
/* `steps` steps of the Chebyshev iteration for M_l y = b on [lo, hi] with the iterates in B[0], B[1]: from zero when from < 0 (the
 * result in B[to]), else from B[from].  Returns the index of the panel that holds the last iterate. */
static int mg_cheb(mg_run *r, int l, double lo, double hi, int steps, const char *b, int64_t lb, char *const B[2], const int64_t LB[2],
      int from, int to) {
   const double scale = r->op->mg_scale, shift = r->op->mg_shift, tb = 0.5 * (hi + lo), dl = 0.5 * (hi - lo);
   hipk_cheb_coef cf;
   memset(&cf, 0, sizeof(cf));
   if (from < 0 && (steps == 1 || !(dl > 0.0))) {               /* y_1 = b / tb (a one-point level: the exact solution) */
      for (int c = 0; c < r->nc; c++) cf.cx[c] = 1.0 / tb;
      mg_step(r, l, &cf, b, lb, NULL, 0, NULL, 0, B[to], LB[to]);
      return to;
   }
   double rho = dl / tb;
   if (from < 0) {
      /* as in primme_amd_chebyshev_precond: y_1 = b / tb is never stored, step k = 1 .. steps - 1 writes y_{k+1} */
      for (int k = 1; k < steps; k++) {
         const int o = (to + (steps - 1 - k)) % 2;
         for (int c = 0; c < r->nc; c++) {
            double rc = rho;
            cheb_step_coef(tb, dl, -shift, k, &rc, &cf, c);
            cf.cw[c] *= scale;
            if (c == r->nc - 1) rho = rc;
         }
         const char *yk = k == 1 ? b : B[1 - o], *yp = k == 1 ? NULL : (k == 2 ? b : B[o]);
         mg_step(r, l, &cf, b, lb, yk, k == 1 ? lb : LB[1 - o], yp, k == 2 ? lb : LB[o], B[o], LB[o]);
      }
      return to;
   }
   /* from y_0 = B[from]: y_1 = y_0 + (b - M y_0) / tb, then the three-term steps; y_j goes to B[(from + j) % 2] */
   for (int j = 1; j <= steps; j++) {
      const int o = (from + j) % 2;
      double cy, cp, cx, cw;
      if (j == 1 || !(dl > 0.0)) { cy = 1.0 - shift / tb; cp = 0.0; cx = 1.0 / tb; cw = -scale / tb; }
      else {
         const double rn = 1.0 / (2.0 * tb / dl - rho), a = rn * rho, bb = 2.0 * rn / dl;
         cy = 1.0 + a - bb * shift; cp = -a; cx = bb; cw = -bb * scale;
         rho = rn;
      }
      for (int c = 0; c < r->nc; c++) { cf.cy[c] = cy; cf.cp[c] = cp; cf.cx[c] = cx; cf.cw[c] = cw; }
      mg_step(r, l, &cf, b, lb, B[1 - o], LB[1 - o], (j == 1 || cp == 0.0) ? NULL : B[o], LB[o], B[o], LB[o]);
   }
   return (from + steps) % 2;
}
/* panel q (0: right-hand side, 1, 2: iterates) of level l >= 1; level 0 has only its temporary, q = 0 */
static char *mg_panel(const primme_amd_operator *op, size_t es, int l, int q) {
   size_t off = 0;
   for (int k = 0; k < l; k++) off += (size_t)op->mg_ld[k] * (k == 0 ? 1 : 3);
   return (char *)op->mg_buf + (off + (size_t)op->mg_ld[l] * q) * op->mg_cols * es;
}
/* the cycle at level l for the right-hand side b; the result goes to B[to] */
static void mg_vcycle(mg_run *r, int l, const char *b, int64_t lb, char *const B[2], const int64_t LB[2], int to) {
   primme_amd_operator *op = r->op;
   double lo, hi;
   int D;
   mg_level_ends(op, l, &lo, &hi, &D);
   if (l == op->mg_nlev - 1) { (void)mg_cheb(r, l, lo, hi, op->mg_cs, b, lb, B, LB, -1, to); return; }
   const double slo = hi / (2.0 * D);
   const int a = (to + op->mg_nu) % 2;             /* the pre-smoothed iterate: nu post-smoothing steps later it is in B[to] */
   (void)mg_cheb(r, l, slo, hi, op->mg_nu, b, lb, B, LB, -1, a);
   hipk_cheb_coef cf;                              /* the residual b - M y into the other panel */
   memset(&cf, 0, sizeof(cf));
   for (int c = 0; c < r->nc; c++) { cf.cx[c] = 1.0; cf.cy[c] = -op->mg_shift; cf.cw[c] = -op->mg_scale; }
   mg_step(r, l, &cf, b, lb, B[a], LB[a], NULL, 0, B[1 - a], LB[1 - a]);
   char *bc = mg_panel(op, r->es, l + 1, 0);
   char *const Bc[2] = {mg_panel(op, r->es, l + 1, 1), mg_panel(op, r->es, l + 1, 2)};
   const int64_t ldc = op->mg_ld[l + 1], LBc[2] = {ldc, ldc};
   if (!r->rc) { r->rc = hipk_mg_restrict(r->stream, r->dt, op->mg_n[l], op->mg_n[l + 1], r->nc, B[1 - a], LB[1 - a], bc, ldc); g_mg_launches++; }
   mg_vcycle(r, l + 1, bc, ldc, Bc, LBc, 0);
   if (!r->rc) { r->rc = hipk_mg_prolong_add(r->stream, r->dt, op->mg_n[l], op->mg_n[l + 1], r->nc, Bc[0], ldc, B[a], LB[a]); g_mg_launches++; }
   (void)mg_cheb(r, l, slo, hi, op->mg_nu, b, lb, B, LB, a, to);
}

extern "C" void primme_amd_multigrid_precond(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy,
      int *blockSize, struct primme_params *primme, int *ierr) {
   primme_amd_operator *op = (primme_amd_operator *)primme->preconditioner;
   void *stream = primme->queue ? (void *)*(hipStream_t *)primme->queue : NULL;
   if (!op || op->mg_nlev < 1) { *ierr = 1; return; }
   *ierr = 0;
   if (*blockSize <= 0) return;
   if (!stream) stream = hipk_ctx_stream(hipk_csr_ctx(op->A));
   mg_run r;
   r.op = op; r.stream = stream; r.dt = hipk_csr_dtype(op->A); r.es = op_elem(r.dt); r.rc = 0;
   const int want = *blockSize < HIPK_CHEB_MAXCOLS ? *blockSize : HIPK_CHEB_MAXCOLS;
   if (want > op->mg_cols) {                       /* scratch for the widest chunk seen */
      if (op->mg_buf) (void)hipFree(op->mg_buf);
      op->mg_buf = NULL; op->mg_cols = 0;
      size_t elems = (size_t)op->mg_ld[0];
      for (int l = 1; l < op->mg_nlev; l++) elems += 3 * (size_t)op->mg_ld[l];
      if (hipMalloc(&op->mg_buf, elems * r.es * want) != hipSuccess) { *ierr = 1; return; }
      op->mg_cols = want;
   }
   for (int c0 = 0; c0 < *blockSize && !r.rc; c0 += HIPK_CHEB_MAXCOLS) {
      r.nc = *blockSize - c0 < HIPK_CHEB_MAXCOLS ? *blockSize - c0 : HIPK_CHEB_MAXCOLS;
      const char *xc = (const char *)x + (size_t)c0 * *ldx * r.es;
      char *const B[2] = {(char *)y + (size_t)c0 * *ldy * r.es, mg_panel(op, r.es, 0, 0)};
      const int64_t LB[2] = {*ldy, op->mg_ld[0]};
      g_mg_applies += r.nc;
      mg_vcycle(&r, 0, xc, *ldx, B, LB, 0);
   }
   if (r.rc) *ierr = 1;
}

/* ---- aggregation algebraic multigrid preconditioner for CSR operators (kernels in hipk_amg.hip) ----------
 * y = K^-1 x: one symmetric V(nu, nu) cycle from zero for M = A + shift I on the hierarchy of primme_amd_amg_plan_create,
 *    vcycle(l, b):  l == last: G b (at most PRIMME_AMD_AMG_DENSE_ROWS rows) or nu_c Chebyshev steps from zero
 *                   y = nu Chebyshev steps from zero;  y += over P vcycle(l + 1, P' (b - M_l y));  nu Chebyshev steps from y
 * The Chebyshev iteration is the one for D_l^-1 M_l on [rho_l / 4, rho_l]: y_1 = D^-1 b / tb, then
 *    y_{k+1} = y_k + a (y_k - y_{k-1}) + bb D^-1 (b - M y_k),  a = rho_{k+1} rho_k, bb = 2 rho_{k+1} / dl,
 * and started at y: y_1 = y + D^-1 (b - M y) / tb, which returns y + p(D^-1 M) D^-1 (b - M y) with the smoother's own
 * polynomial p and makes K symmetric (the construction of 4n).  A step is the level product (hipk_csr_matvec; level 0 the
 * operator's own matrix, hipk_csr_matvec_shifted adding the shift) and one hipk_amg_smooth_update.  The iterates of a level
 * alternate between two panels, y_{k+1} over y_{k-1}; a sequence starts in the panel that makes its last iterate land where
 * the next stage expects it (the result of a level in panel 0; level 0: the caller's y).
 * With the hierarchy of primme_amd_amg_plan_create_smoothed the restriction and the interpolation of a level
 * are hipk_amg_csr_apply on R_l = P_l' and P_l, over = 1; everything else is the same. */
static long g_amg_applies, g_amg_launches, g_amg_levels;
extern "C" void primme_amd_amg_stats(long *applies, long *launches, long *levels) {
   if (applies) *applies = g_amg_applies;
   if (launches) *launches = g_amg_launches;
   if (levels) *levels = g_amg_levels;             /* of the hierarchy applied last */
   g_amg_applies = g_amg_launches = g_amg_levels = 0;
}

static double amg_now(void) { struct timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
static void amg_free_dev(void *pp) {
   void **p = (void **)pp;
   if (*p) (void)hipFree(*p);
   *p = NULL;
}
/* the CSR arrays of a level's matrix and, with all = 1, everything else the level holds */
static void amg_level_release(amg_level_dev *L, int all) {
   amg_free_dev(&L->mrp); amg_free_dev(&L->mci); amg_free_dev(&L->mva);
   if (!all) return;
   for (int k = 0; k < 2; k++)
      if (L->M[k]) { (void)hipk_csr_destroy(L->M[k]); L->M[k] = NULL; }
   amg_free_dev(&L->dinv); amg_free_dev(&L->agg); amg_free_dev(&L->aggptr); amg_free_dev(&L->aggrows);
   amg_free_dev(&L->prp); amg_free_dev(&L->pci); amg_free_dev(&L->pva); amg_free_dev(&L->rrp); amg_free_dev(&L->rci); amg_free_dev(&L->rva);
}
static void amg_hierarchy_unref(primme_amd_amg_hierarchy *h) {
   if (!h || --h->refs > 0) return;
   for (int l = 0; l < PRIMME_AMD_AMG_MAXLEVELS; l++) amg_level_release(&h->lv[l], 1);
   amg_free_dev(&h->G);
   if (h->own_ctx && h->ctx) (void)hipk_ctx_destroy(h->ctx);
   free(h);
}
static void amg_release(amg_state *s) {
   if (s->buf) (void)hipFree(s->buf);
   amg_hierarchy_unref(s->h);
   memset(s, 0, sizeof(*s));
}
/* a device copy of `bytes` host bytes; 0 on success */
static int amg_to_device(hipk_ctx *ctx, void **dst, const void *src, size_t bytes) {
   if (hipMalloc(dst, bytes ? bytes : 1) != hipSuccess) { *dst = NULL; return -2; }
   return bytes ? hipk_upload(ctx, *dst, src, bytes) : 0;
}
/* a host copy of `count` elements of a device array; NULL: no memory or the copy failed */
template <typename T> static T *amg_to_host(hipk_ctx *ctx, const T *src, int64_t count) {
   T *dst = (T *)malloc(sizeof(T) * (size_t)(count > 0 ? count : 1));
   if (dst && count > 0 && hipk_download(ctx, dst, src, sizeof(T) * (size_t)count)) { free(dst); dst = NULL; }
   return dst;
}

/* the operator of a level for panels of type dti (0 double, 1 float) from the level's host CSR arrays in double */
static int amg_level_operator(hipk_ctx *ctx, int dti, int64_t n, int64_t nnz, const int32_t *rp, const int32_t *ci, const double *va, hipk_csr **M) {
   if (dti == 0) return hipk_csr_create(ctx, HIPK_F64, n, n, 0, rp, ci, va, M);
   float *vf = (float *)malloc(sizeof(float) * (size_t)(nnz > 0 ? nnz : 1));
   if (!vf) return -2;
   for (int64_t q = 0; q < nnz; q++) vf[q] = (float)va[q];
   const int rc = hipk_csr_create(ctx, HIPK_F32, n, n, 0, rp, ci, vf, M);
   free(vf);
   return rc;
}

/* level l of the host plan P on the device: dinv, the matrix (l >= 1), the aggregate maps and the transfer matrices */
static int amg_upload_level(primme_amd_amg_hierarchy *h, int l, const primme_amd_amg_plan *P) {
   const primme_amd_amg_level *H = &P->level[l];
   const primme_amd_amg_transfer *X = &P->transfer[l];
   amg_level_dev *L = &h->lv[l];
   hipk_ctx *ctx = h->ctx;
   L->n = H->n; L->nc = H->nc; L->nnz = H->nnz; L->rho = H->rho; L->ld = (H->n + 3) / 4 * 4; L->pnnz = 0;
   int rc = L->dinv ? 0 : amg_to_device(ctx, (void **)&L->dinv, H->dinv, sizeof(double) * (size_t)H->n);
   if (!rc && l > 0 && h->priv) {
      if (!L->M[h->priv - 1]) rc = amg_level_operator(ctx, h->priv - 1, H->n, H->nnz, H->rowptr, H->colind, H->values, &L->M[h->priv - 1]);
   } else if (!rc && l > 0 && !L->mrp) {
      rc = amg_to_device(ctx, (void **)&L->mrp, H->rowptr, sizeof(int32_t) * (size_t)(H->n + 1));
      if (!rc) rc = amg_to_device(ctx, (void **)&L->mci, H->colind, sizeof(int32_t) * (size_t)H->nnz);
      if (!rc) rc = amg_to_device(ctx, (void **)&L->mva, H->values, sizeof(double) * (size_t)H->nnz);
   }
   if (!rc && H->nc > 0 && !L->agg) {
      rc = amg_to_device(ctx, (void **)&L->agg, H->agg, sizeof(int32_t) * (size_t)H->n);
      if (!rc) rc = amg_to_device(ctx, (void **)&L->aggptr, H->aggptr, sizeof(int32_t) * (size_t)(H->nc + 1));
      if (!rc) rc = amg_to_device(ctx, (void **)&L->aggrows, H->aggrows, sizeof(int32_t) * (size_t)H->n);
   }
   if (!rc && H->nc > 0 && X->prowptr) {
      L->pnnz = X->pnnz;
      rc = amg_to_device(ctx, (void **)&L->prp, X->prowptr, sizeof(int32_t) * (size_t)(H->n + 1));
      if (!rc) rc = amg_to_device(ctx, (void **)&L->pci, X->pcolind, sizeof(int32_t) * (size_t)X->pnnz);
      if (!rc) rc = amg_to_device(ctx, (void **)&L->pva, X->pvalues, sizeof(double) * (size_t)X->pnnz);
      if (!rc) rc = amg_to_device(ctx, (void **)&L->rrp, X->rrowptr, sizeof(int32_t) * (size_t)(H->nc + 1));
      if (!rc) rc = amg_to_device(ctx, (void **)&L->rci, X->rcolind, sizeof(int32_t) * (size_t)X->pnnz);
      if (!rc) rc = amg_to_device(ctx, (void **)&L->rva, X->rvalues, sizeof(double) * (size_t)X->pnnz);
   }
   return rc;
}

/* the operators of the levels >= 1 for panels of type dti (0 double, 1 float), from the levels' CSR arrays */
static int amg_level_operators(primme_amd_amg_hierarchy *h, int dti) {
   int rc = 0;
   for (int l = 1; l < h->nlev && !rc; l++) {
      amg_level_dev *L = &h->lv[l];
      if (L->M[dti]) continue;
      if (!L->mrp) return -1;                      /* a private hierarchy serves the operator type it was made for */
      int32_t *rp = amg_to_host(h->ctx, L->mrp, L->n + 1), *ci = amg_to_host(h->ctx, L->mci, L->nnz);
      double *va = amg_to_host(h->ctx, L->mva, L->nnz);
      rc = (rp && ci && va) ? amg_level_operator(h->ctx, dti, L->n, L->nnz, rp, ci, va, &L->M[dti]) : -2;
      free(rp); free(ci); free(va);
   }
   return rc;
}

/* The smoothed set-up with its row-parallel stages on the device (hipk_amg_setup.hip).  Per level: the host
 * aggregates M_l (pa_amg_level_aggregate: the passes of 4o, untouched), the maps are uploaded, the device builds P_l, R_l,
 * M_{l+1}, dinv_{l+1} and rho_{l+1}, and M_{l+1} with its diagonal comes back for the next aggregation and stays resident.
 * A stage that answers 1 (a count beyond the entry limit, no device memory) sends the LEVEL to the host routines
 * (pa_amg_prolongation, pa_amg_galerkin_general), whose results are uploaded, and the build goes on.  P keeps the host side of
 * the build: the level matrices always, transfer matrices only where a level fell back. */
static int amg_build_device(primme_amd_amg_hierarchy *h, primme_amd_amg_plan *P, int64_t n, const int32_t *rowptr, const int32_t *colind,
      const void *values, size_t elem_size) {
   double *dg = (double *)malloc(sizeof(double) * (size_t)n);
   int32_t *tmp = (int32_t *)malloc(sizeof(int32_t) * (size_t)n);
   void *st = hipk_ctx_stream(h->ctx);
   int rc = (dg && tmp) ? 0 : -5;
   if (!rc) rc = pa_amg_level0(n, rowptr, colind, values, elem_size, h->shift, &P->level[0], dg);
   if (!rc) {                                      /* level 0 in double beside the operator's own copy, until level 1 stands */
      const primme_amd_amg_level *H = &P->level[0];
      amg_level_dev *L = &h->lv[0];
      rc = amg_to_device(h->ctx, (void **)&L->mrp, H->rowptr, sizeof(int32_t) * (size_t)(n + 1));
      if (!rc) rc = amg_to_device(h->ctx, (void **)&L->mci, H->colind, sizeof(int32_t) * (size_t)H->nnz);
      if (!rc) rc = amg_to_device(h->ctx, (void **)&L->mva, H->values, sizeof(double) * (size_t)H->nnz);
   }
   int l = 0;
   while (!rc) {
      primme_amd_amg_level *H = &P->level[l], *Hn = &P->level[l + 1];
      amg_level_dev *L = &h->lv[l], *N = &h->lv[l + 1];
      if (H->n <= PRIMME_AMD_AMG_DENSE_ROWS || l + 1 >= PRIMME_AMD_AMG_MAXLEVELS) break;
      double t = amg_now();
      rc = pa_amg_level_aggregate(H, dg, h->theta, tmp);
      h->stage[l][0] = amg_now() - t;
      if (rc) { rc = rc > 0 ? 0 : rc; break; }     /* 1: stalled, this level is the last */
      rc = amg_upload_level(h, l, P);              /* dinv (level 0) and the aggregate maps */
      if (rc) break;
      const int64_t nc = H->nc;
      int64_t pnnz = 0, cnnz = 0;
      double *diag = NULL, rho = 0.0;
      int flag = 0;
      const double t0 = amg_now();
      int drc = hipk_amg_build_prolongation(st, H->n, nc, L->mrp, L->mci, L->mva, L->dinv, L->agg, h->omega / H->rho, h->max_entries, &L->prp, &L->pci, &L->pva, &pnnz);
      const double t1 = amg_now();
      if (!drc) drc = hipk_amg_csr_transpose(st, H->n, nc, pnnz, L->prp, L->pci, L->pva, h->max_entries, &L->rrp, &L->rci, &L->rva);
      const double t2 = amg_now();
      if (!drc) drc = hipk_amg_galerkin(st, H->n, nc, L->mrp, L->mci, L->mva, L->prp, L->pci, L->pva, L->rrp, L->rci, L->rva, h->max_entries, &N->mrp, &N->mci, &N->mva, &cnnz);
      const double t3 = amg_now();
      if (!drc && (hipMalloc((void **)&N->dinv, sizeof(double) * (size_t)nc) != hipSuccess || hipMalloc((void **)&diag, sizeof(double) * (size_t)nc) != hipSuccess)) {
         (void)hipGetLastError();
         drc = 1;
      }
      if (!drc) drc = hipk_amg_level_finish(st, nc, N->mrp, N->mci, N->mva, N->dinv, diag, &rho, &flag);
      const double t4 = amg_now();
      if (!drc && flag) rc = -1;                   /* a row of M_{l+1} without a diagonal entry, or m_ii <= 0 */
      if (!drc && !rc) {
         L->pnnz = pnnz;
         Hn->n = nc; Hn->nnz = cnnz; Hn->rho = rho;
         Hn->rowptr = amg_to_host(h->ctx, N->mrp, nc + 1);
         Hn->colind = amg_to_host(h->ctx, N->mci, cnnz);
         Hn->values = amg_to_host(h->ctx, N->mva, cnnz);
         Hn->dinv = amg_to_host(h->ctx, N->dinv, nc);
         if (!Hn->rowptr || !Hn->colind || !Hn->values || !Hn->dinv || hipk_download(h->ctx, dg, diag, sizeof(double) * (size_t)nc)) rc = -5;
         N->n = nc; N->nnz = cnnz; N->rho = rho; N->ld = (nc + 3) / 4 * 4;
         h->stage[l][1] = t1 - t0; h->stage[l][2] = t2 - t1; h->stage[l][3] = t3 - t2; h->stage[l][4] = t4 - t3; h->stage[l][5] = amg_now() - t4;
         h->device_seconds += t4 - t0;
      }
      amg_free_dev(&diag);
      if (drc < 0) rc = -1;
      if (drc == 1) {                              /* the level on the host, nothing of the device's attempt kept */
         amg_free_dev(&L->prp); amg_free_dev(&L->pci); amg_free_dev(&L->pva); amg_free_dev(&L->rrp); amg_free_dev(&L->rci); amg_free_dev(&L->rva);
         amg_level_release(N, 1);
         /* the same lines of the stage table: P with its transpose, the triple product, the finish, and the upload in the
            place of the download */
         const double h0 = amg_now();
         rc = pa_amg_prolongation(H, h->omega, &P->transfer[l]);
         const double h1 = amg_now();
         if (!rc) rc = pa_amg_galerkin_general(H, &P->transfer[l], Hn);
         const double h2 = amg_now();
         if (!rc) rc = pa_amg_level_finish(Hn, dg);
         const double h3 = amg_now();
         if (!rc) rc = amg_upload_level(h, l, P);
         if (!rc) rc = amg_upload_level(h, l + 1, P);
         h->stage[l][1] = h1 - h0; h->stage[l][2] = 0.0; h->stage[l][3] = h2 - h1; h->stage[l][4] = h3 - h2; h->stage[l][5] = amg_now() - h3;
         h->fallback++;
      }
      if (l == 0) amg_level_release(L, 0);         /* level 0 runs on the operator it is attached to */
      l++;
   }
   if (!rc && h->lv[0].mrp) amg_level_release(&h->lv[0], 0);
   if (!rc && l == 0) rc = amg_upload_level(h, 0, P);                      /* one level: dinv */
   free(dg); free(tmp);
   P->nlevels = l + 1;
   return rc;
}

/* priv = 1: the private hierarchy of set_amg[_smoothed]: the host route under the operator's own context, which outlives it,
   the level operators of the operator's type made straight from the host plan.  Never handed to a caller. */
static int amg_hierarchy_build(primme_amd_operator *op, const int32_t *rowptr_host, const int32_t *colind_host,
      const void *values_host, int smoothed, double theta, double omega, double shift, int setup, int priv, primme_amd_amg_hierarchy **out) {
   if (out) *out = NULL;
   if (!op || !out) return -1;
   const hipk_dtype dt = hipk_csr_dtype(op->A);
   if (op->mode != 0 || (op->comm && primme_amd_comm_size(op->comm) > 1) || op->ldscale != 1 || (dt != HIPK_F64 && dt != HIPK_F32)) return -44;
   if (hipk_csr_kind(op->A) != 0 || op->lo > 0 || op->hi > 0) return -44;          /* a stencil has ("multigrid", ...) */
   if (setup != 0 && setup != 1) return -1;
   if (setup == 1 && !smoothed) return -44;        /* the plain set-up is the sequential aggregation: the host route only */
   if (!rowptr_host || !colind_host || !values_host || !(theta >= 0.0 && theta < 1.0) || !(shift >= 0.0)) return -1;
   if (smoothed && !(omega > 0.0 && omega < 2.0)) return -1;
   const int64_t n = hipk_csr_nrows(op->A);
   if (n < 1 || rowptr_host[0] != 0 || (int64_t)rowptr_host[n] != hipk_csr_nnz(op->A)) return -1;
   const size_t es = dt == HIPK_F64 ? 8 : 4;
   const double t0 = amg_now();
   primme_amd_amg_hierarchy *h = (primme_amd_amg_hierarchy *)calloc(1, sizeof(*h));
   if (!h) return -1;
   h->refs = 1; h->smoothed = smoothed != 0; h->shift = shift; h->theta = theta; h->omega = smoothed ? omega : 0.0;
   h->n0 = n; h->nnz0 = rowptr_host[n];
   h->max_entries = INT32_MAX;
   if (setup == 1) {
      /* PRIMME_AMD_AMG_SETUP_MAX_ENTRIES lowers the entry limit beyond which a level is built by the host routines (the
         tests reach that path with it; read when a hierarchy is created) */
      const char *e = getenv("PRIMME_AMD_AMG_SETUP_MAX_ENTRIES");
      if (e && *e) { const long long v = atoll(e); if (v >= 0 && v < INT32_MAX) h->max_entries = v; }
   }
   if (priv) { h->ctx = hipk_csr_ctx(op->A); h->priv = 1 + (dt == HIPK_F64 ? 0 : 1); }
   else if (hipk_ctx_create(&h->ctx, NULL)) { free(h); return -1; }
   else h->own_ctx = 1;
   primme_amd_amg_plan *P = NULL;
   int rc = 0;
   if (setup == 1) {
      P = (primme_amd_amg_plan *)calloc(1, sizeof(*P));
      rc = P ? amg_build_device(h, P, n, rowptr_host, colind_host, values_host, es) : -5;
   } else {
      rc = smoothed ? primme_amd_amg_plan_create_smoothed(n, rowptr_host, colind_host, values_host, es, shift, theta, omega, &P)
                    : primme_amd_amg_plan_create(n, rowptr_host, colind_host, values_host, es, shift, theta, &P);
      for (int l = 0; !rc && l < P->nlevels; l++) rc = amg_upload_level(h, l, P);
   }
   if (!rc) {
      h->nlev = P->nlevels;
      const int64_t nl = P->level[P->nlevels - 1].n;
      if (nl <= PRIMME_AMD_AMG_DENSE_ROWS) {
         double *G = (double *)malloc(sizeof(double) * (size_t)(nl * nl));
         rc = G ? primme_amd_amg_coarse_inverse(P, G) : -2;             /* -1: the matrix is not positive definite */
         if (!rc) rc = amg_to_device(h->ctx, (void **)&h->G, G, sizeof(double) * (size_t)(nl * nl));
         free(G);
      }
   }
   primme_amd_amg_plan_free(P);
   if (rc) { amg_hierarchy_unref(h); return -1; }
   h->setup_seconds = amg_now() - t0;
   *out = h;
   return 0;
}

extern "C" int primme_amd_amg_hierarchy_create(primme_amd_operator *op, const int32_t *rowptr_host, const int32_t *colind_host,
      const void *values_host, int smoothed, double theta, double omega, double shift, int setup, primme_amd_amg_hierarchy **out) {
   return amg_hierarchy_build(op, rowptr_host, colind_host, values_host, smoothed, theta, omega, shift, setup, 0, out);
}

extern "C" void primme_amd_amg_hierarchy_destroy(primme_amd_amg_hierarchy *h) { amg_hierarchy_unref(h); }

extern "C" int primme_amd_operator_set_amg_hierarchy(primme_amd_operator *op, primme_amd_amg_hierarchy *h, int smooth_steps, int coarse_steps,
      double over) {
   if (!op || !h) return -1;
   const hipk_dtype dt = hipk_csr_dtype(op->A);
   if (op->mode != 0 || (op->comm && primme_amd_comm_size(op->comm) > 1) || op->ldscale != 1 || (dt != HIPK_F64 && dt != HIPK_F32)) return -44;
   if (hipk_csr_kind(op->A) != 0 || op->lo > 0 || op->hi > 0) return -44;
   if (smooth_steps < 1 || coarse_steps < 1 || !(over >= 1.0 && over < 2.0) || (h->smoothed && over != 1.0)) return -1;
   if (hipk_csr_nrows(op->A) != h->n0 || hipk_csr_nnz(op->A) != h->nnz0) return -1;
   const int dti = dt == HIPK_F64 ? 0 : 1;
   if (amg_level_operators(h, dti)) return -1;
   h->refs++;                                       /* before the release: h may be the hierarchy attached now */
   h->attached++;
   amg_release(&op->amg);
   op->amg.h = h; op->amg.dti = dti; op->amg.nu = smooth_steps; op->amg.cs = coarse_steps; op->amg.over = over;
   return 0;
}

extern "C" int primme_amd_amg_hierarchy_info(const primme_amd_amg_hierarchy *h, int *nlevels, int64_t *rows, int64_t *nnz, int64_t *pnnz,
      double *setup_seconds, double *device_seconds, long *times_attached) {
   if (!h) return -1;
   if (nlevels) *nlevels = h->nlev;
   for (int l = 0; l < PRIMME_AMD_AMG_MAXLEVELS; l++) {
      if (rows) rows[l] = l < h->nlev ? h->lv[l].n : 0;
      if (nnz) nnz[l] = l < h->nlev ? (l == 0 ? h->nnz0 : h->lv[l].nnz) : 0;
      if (pnnz) pnnz[l] = l < h->nlev ? h->lv[l].pnnz : 0;
   }
   if (setup_seconds) *setup_seconds = h->setup_seconds;
   if (device_seconds) *device_seconds = h->device_seconds;
   if (times_attached) *times_attached = h->attached;
   return 0;
}

extern "C" int primme_amd_amg_hierarchy_stages(const primme_amd_amg_hierarchy *h, int *fallback_levels, double *seconds) {
   if (!h) return -1;
   if (fallback_levels) *fallback_levels = h->fallback;
   if (seconds) memcpy(seconds, h->stage, sizeof(h->stage));
   return 0;
}

extern "C" int primme_amd_amg_hierarchy_download(const primme_amd_amg_hierarchy *h, primme_amd_amg_plan **plan) {
   if (plan) *plan = NULL;
   if (!h || !plan) return -1;
   primme_amd_amg_plan *P = (primme_amd_amg_plan *)calloc(1, sizeof(*P));
   if (!P) return -5;
   int ok = 1;
   P->nlevels = h->nlev; P->shift = h->shift; P->theta = h->theta; P->omega = h->omega;
   for (int l = 0; l < h->nlev && ok; l++) {
      const amg_level_dev *L = &h->lv[l];
      primme_amd_amg_level *H = &P->level[l];
      primme_amd_amg_transfer *X = &P->transfer[l];
      H->n = L->n; H->nc = L->nc; H->rho = L->rho; H->nnz = l == 0 ? h->nnz0 : L->nnz;
      ok = (H->dinv = amg_to_host(h->ctx, L->dinv, L->n)) != NULL;
      if (ok && l > 0) ok = (H->rowptr = amg_to_host(h->ctx, L->mrp, L->n + 1)) && (H->colind = amg_to_host(h->ctx, L->mci, L->nnz)) &&
                            (H->values = amg_to_host(h->ctx, L->mva, L->nnz));
      if (ok && L->nc > 0) ok = (H->agg = amg_to_host(h->ctx, L->agg, L->n)) && (H->aggptr = amg_to_host(h->ctx, L->aggptr, L->nc + 1)) &&
                                (H->aggrows = amg_to_host(h->ctx, L->aggrows, L->n));
      if (ok && L->prp) {
         X->pnnz = L->pnnz;
         ok = (X->prowptr = amg_to_host(h->ctx, L->prp, L->n + 1)) && (X->pcolind = amg_to_host(h->ctx, L->pci, L->pnnz)) &&
              (X->pvalues = amg_to_host(h->ctx, L->pva, L->pnnz)) && (X->rrowptr = amg_to_host(h->ctx, L->rrp, L->nc + 1)) &&
              (X->rcolind = amg_to_host(h->ctx, L->rci, L->pnnz)) && (X->rvalues = amg_to_host(h->ctx, L->rva, L->pnnz));
      }
   }
   if (!ok) { primme_amd_amg_plan_free(P); return -5; }
   *plan = P;
   return 0;
}

/* omega = 0: plain aggregation with the over-correction `over`; omega in (0, 2): smoothed aggregation, over = 1 */
static int amg_configure(primme_amd_operator *op, const int32_t *rowptr_host, const int32_t *colind_host,
      const void *values_host, int smooth_steps, int coarse_steps, double theta, double over, double omega, double shift) {
   if (!op) return -1;
   const hipk_dtype dt = hipk_csr_dtype(op->A);
   if (op->mode != 0 || (op->comm && primme_amd_comm_size(op->comm) > 1) || op->ldscale != 1 || (dt != HIPK_F64 && dt != HIPK_F32)) return -44;
   if (hipk_csr_kind(op->A) != 0 || op->lo > 0 || op->hi > 0) return -44;          /* a stencil has ("multigrid", ...) */
   if (!rowptr_host || !colind_host || !values_host || smooth_steps < 1 || coarse_steps < 1 || !(theta >= 0.0 && theta < 1.0) ||
       !(over >= 1.0 && over < 2.0) || !(shift >= 0.0)) return -1;
   const int64_t n = hipk_csr_nrows(op->A);
   if (n < 1 || rowptr_host[0] != 0 || (int64_t)rowptr_host[n] != hipk_csr_nnz(op->A)) return -1;
   /* a private hierarchy: created, attached, and destroyed with the operator, which then holds its only reference.  The
      operator changes only when everything is in order */
   primme_amd_amg_hierarchy *h = NULL;
   if (amg_hierarchy_build(op, rowptr_host, colind_host, values_host, omega != 0.0, theta, omega, shift, 0, 1, &h)) return -1;
   const int rc = primme_amd_operator_set_amg_hierarchy(op, h, smooth_steps, coarse_steps, over);
   primme_amd_amg_hierarchy_destroy(h);
   return rc ? -1 : 0;
}

extern "C" int primme_amd_operator_set_amg(primme_amd_operator *op, const int32_t *rowptr_host, const int32_t *colind_host,
      const void *values_host, int smooth_steps, int coarse_steps, double theta, double over, double shift) {
   return amg_configure(op, rowptr_host, colind_host, values_host, smooth_steps, coarse_steps, theta, over, 0.0, shift);
}

extern "C" int primme_amd_operator_set_amg_smoothed(primme_amd_operator *op, const int32_t *rowptr_host, const int32_t *colind_host,
      const void *values_host, int smooth_steps, int coarse_steps, double theta, double omega, double shift) {
   if (!(omega > 0.0 && omega < 2.0)) return -1;
   return amg_configure(op, rowptr_host, colind_host, values_host, smooth_steps, coarse_steps, theta, 1.0, omega, shift);
}

struct amg_run {
   primme_amd_operator *op;
   void *stream;
   hipk_dtype dt;
   size_t es;
   int nc;
   int rc;
};
/* W = M_l Y */
static void amg_product(amg_run *r, int l, const char *y, int64_t ldy, char *w, int64_t ldw) {
   if (r->rc) return;
   amg_state *s = &r->op->amg;
   if (l > 0) r->rc = hipk_csr_matvec(s->h->lv[l].M[s->dti], r->stream, y, ldy, w, ldw, r->nc);
   else if (s->h->shift == 0.0) r->rc = hipk_csr_matvec(r->op->A, r->stream, y, ldy, w, ldw, r->nc);
   else {
      double ms[HIPK_CHEB_MAXCOLS];
      for (int c = 0; c < r->nc; c++) ms[c] = -s->h->shift;
      r->rc = hipk_csr_matvec_shifted(r->op->A, r->stream, y, ldy, w, ldw, r->nc, ms);
   }
   g_amg_launches++;
}
static void amg_update(amg_run *r, int l, const hipk_cheb_coef *cf, int with_dinv, const char *x, int64_t ldx, const char *w, int64_t ldw,
      const char *yk, int64_t ldk, const char *yp, int64_t ldp, char *out, int64_t ldo) {
   if (r->rc) return;
   const amg_level_dev *L = &r->op->amg.h->lv[l];
   r->rc = hipk_amg_smooth_update(r->stream, r->dt, L->n, r->nc, cf, with_dinv ? L->dinv : NULL, x, ldx, w, ldw, yk, ldk, yp, ldp, out, ldo);
   g_amg_launches++;
}
/* `steps` steps of the Chebyshev iteration for D^-1 M_l y = D^-1 b on [rho_l / 4, rho_l] with the iterates in Y[0], Y[1] and the
 * product in W: from zero when from < 0 (the result in Y[to]), else from Y[from].  Returns the panel of the last iterate. */
static int amg_cheb(amg_run *r, int l, int steps, const char *b, int64_t lb, char *const Y[2], const int64_t LY[2], char *W, int64_t ldw,
      int from, int to) {
   const double hi = r->op->amg.h->lv[l].rho, lo = 0.25 * hi, tb = 0.5 * (hi + lo), dl = 0.5 * (hi - lo);
   hipk_cheb_coef cf;
   double rho = dl / tb;
   int cur, first = 1;
   memset(&cf, 0, sizeof(cf));
   if (from < 0) {
      cur = ((to - (steps - 1)) % 2 + 2) % 2;
      for (int c = 0; c < r->nc; c++) cf.cx[c] = 1.0 / tb;
      amg_update(r, l, &cf, 1, b, lb, NULL, 0, NULL, 0, NULL, 0, Y[cur], LY[cur]);
      steps--;
      first = 0;
   } else cur = from;
   for (int k = 0; k < steps; k++) {
      double cy, cp, cx, cw;
      amg_product(r, l, Y[cur], LY[cur], W, ldw);
      if (first) { cy = 1.0; cp = 0.0; cx = 1.0 / tb; cw = -1.0 / tb; first = 0; }
      else {
         const double rn = 1.0 / (2.0 * tb / dl - rho), a = rn * rho, bb = 2.0 * rn / dl;
         cy = 1.0 + a; cp = -a; cx = bb; cw = -bb;
         rho = rn;
      }
      /* y_0 = 0 has no panel: the second iterate from zero has no y_{k-1} term */
      const int has_prev = cp != 0.0 && !(from < 0 && k == 0);
      for (int c = 0; c < r->nc; c++) { cf.cy[c] = cy; cf.cp[c] = cp; cf.cx[c] = cx; cf.cw[c] = cw; }
      amg_update(r, l, &cf, 1, b, lb, W, ldw, Y[cur], LY[cur], has_prev ? Y[1 - cur] : NULL, LY[1 - cur], Y[1 - cur], LY[1 - cur]);
      cur = 1 - cur;
   }
   return cur;
}
/* panel q of level l: level 0 has q = 0 (iterate) and 1 (product); the others 0 (right-hand side), 1, 2 (iterates), 3 (product) */
static char *amg_panel(const amg_state *s, size_t es, int l, int q) {
   size_t off = 0;
   for (int k = 0; k < l; k++) off += (size_t)s->h->lv[k].ld * (k == 0 ? 2 : 4);
   return (char *)s->buf + (off + (size_t)s->h->lv[l].ld * q) * s->cols * es;
}
/* the cycle at level l for the right-hand side b; the result goes to Y[0] */
static void amg_vcycle(amg_run *r, int l, const char *b, int64_t lb, char *const Y[2], const int64_t LY[2], char *W, int64_t ldw) {
   amg_state *s = &r->op->amg;
   const amg_level_dev *L = &s->h->lv[l];
   if (l == s->h->nlev - 1) {
      if (s->h->G) {
         if (!r->rc) { r->rc = hipk_amg_dense_apply(r->stream, r->dt, (int)L->n, s->h->G, r->nc, b, lb, Y[0], LY[0]); g_amg_launches++; }
      } else (void)amg_cheb(r, l, s->cs, b, lb, Y, LY, W, ldw, -1, 0);
      return;
   }
   const int a = s->nu % 2;                        /* the pre-smoothed iterate: nu post-smoothing steps later it is in Y[0] */
   (void)amg_cheb(r, l, s->nu, b, lb, Y, LY, W, ldw, -1, a);
   hipk_cheb_coef cf;                              /* the residual b - M y, over the product */
   memset(&cf, 0, sizeof(cf));
   for (int c = 0; c < r->nc; c++) { cf.cx[c] = 1.0; cf.cw[c] = -1.0; }
   amg_product(r, l, Y[a], LY[a], W, ldw);
   amg_update(r, l, &cf, 0, b, lb, W, ldw, NULL, 0, NULL, 0, W, ldw);
   const int64_t ldc = s->h->lv[l + 1].ld, LYc[2] = {ldc, ldc};
   char *bc = amg_panel(s, r->es, l + 1, 0), *Wc = amg_panel(s, r->es, l + 1, 3);
   char *const Yc[2] = {amg_panel(s, r->es, l + 1, 1), amg_panel(s, r->es, l + 1, 2)};
   /* smoothed aggregation: R_l = P_l' and P_l in CSR; plain aggregation: the aggregate maps */
   if (!r->rc) {
      r->rc = L->rrp ? hipk_amg_csr_apply(r->stream, r->dt, L->nc, L->n, L->rrp, L->rci, L->rva, 0, r->nc, W, ldw, bc, ldc)
                     : hipk_amg_restrict(r->stream, r->dt, L->n, L->nc, L->aggptr, L->aggrows, r->nc, W, ldw, bc, ldc);
      g_amg_launches++;
   }
   amg_vcycle(r, l + 1, bc, ldc, Yc, LYc, Wc, ldc);
   if (!r->rc) {
      r->rc = L->prp ? hipk_amg_csr_apply(r->stream, r->dt, L->n, L->nc, L->prp, L->pci, L->pva, 1, r->nc, Yc[0], ldc, Y[a], LY[a])
                     : hipk_amg_prolong_add(r->stream, r->dt, L->n, L->nc, L->agg, s->over, r->nc, Yc[0], ldc, Y[a], LY[a]);
      g_amg_launches++;
   }
   (void)amg_cheb(r, l, s->nu, b, lb, Y, LY, W, ldw, a, 0);
}

extern "C" void primme_amd_amg_precond(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy,
      int *blockSize, struct primme_params *primme, int *ierr) {
   primme_amd_operator *op = (primme_amd_operator *)primme->preconditioner;
   void *stream = primme->queue ? (void *)*(hipStream_t *)primme->queue : NULL;
   if (!op || !op->amg.h) { *ierr = 1; return; }
   *ierr = 0;
   if (*blockSize <= 0) return;
   if (!stream) stream = hipk_ctx_stream(hipk_csr_ctx(op->A));
   amg_state *s = &op->amg;
   amg_run r;
   r.op = op; r.stream = stream; r.dt = hipk_csr_dtype(op->A); r.es = op_elem(r.dt); r.rc = 0;
   const int want = *blockSize < HIPK_CHEB_MAXCOLS ? *blockSize : HIPK_CHEB_MAXCOLS;
   if (want > s->cols) {                           /* scratch for the widest chunk seen */
      if (s->buf) (void)hipFree(s->buf);
      s->buf = NULL; s->cols = 0;
      size_t elems = 2 * (size_t)s->h->lv[0].ld;
      for (int l = 1; l < s->h->nlev; l++) elems += 4 * (size_t)s->h->lv[l].ld;
      if (hipMalloc(&s->buf, elems * r.es * want) != hipSuccess) { *ierr = 1; return; }
      s->cols = want;
   }
   g_amg_levels = s->h->nlev;
   for (int c0 = 0; c0 < *blockSize && !r.rc; c0 += HIPK_CHEB_MAXCOLS) {
      r.nc = *blockSize - c0 < HIPK_CHEB_MAXCOLS ? *blockSize - c0 : HIPK_CHEB_MAXCOLS;
      const char *xc = (const char *)x + (size_t)c0 * *ldx * r.es;
      char *const Y[2] = {(char *)y + (size_t)c0 * *ldy * r.es, amg_panel(s, r.es, 0, 0)};
      const int64_t LY[2] = {*ldy, s->h->lv[0].ld};
      g_amg_applies += r.nc;
      amg_vcycle(&r, 0, xc, *ldx, Y, LY, amg_panel(s, r.es, 0, 1), s->h->lv[0].ld);
   }
   if (r.rc) *ierr = 1;
}

extern "C" int primme_amd_operator_set_complex(primme_amd_operator *op, int on) {
   if (!op) return -1;
   op->ldscale = on ? 2 : 1;
   return 0;
}

extern "C" int primme_amd_operator_set_jacobi(primme_amd_operator *op, int fixed, double shift) {
   if (!op) return -1;
   op->jacobi_fixed = fixed; op->jacobi_shift = shift;
   return 0;
}


/* ---- singular value operator: A and A' both resident in CSR ------------------------------ */
#include "primme_amd_svds.h"
#include "primme_amd_io.h"
struct primme_amd_svds_operator {
   hipk_csr *A, *At;
   primme_amd_comm *comm;        /* NULL: single rank */
   int64_t mLocal, n, nLocal;
   void *full;                   /* n-vector staging (all-gather target / reduce-scatter source) */
   size_t full_cap;
   hipk_dtype dt;
   void *jac_r, *jac_c;          /* Jacobi for the normal equations: row / column sums of squares - shift^2 */
   int cplx;                     /* real-equivalent form of a complex matrix: leading dimensions arrive in complex elements */
   /* Chebyshev polynomial preconditioner (primme_amd_svds_chebyshev_precond): steps = 0 until configured; lo, hi, sigma are the
    * squares of the singular value bounds.  Scratch, side 0 = n-vectors (rows of A'), side 1 = m-vectors (rows of A): two
    * panels of cheb_cols columns each (the iterates, and the product with the first factor for the other side) and, for the
    * unfused path only, the product with the second factor */
   int cheb_steps, cheb_unfused, cheb_fused_all;
   double cheb_lo, cheb_hi, cheb_sigma, cheb_sshift;
   void *cheb_p[2], *cheb_w[2];
   int cheb_cols, cheb_wcols[2];
   int64_t cheb_ld[2];
};

extern "C" int primme_amd_svds_operator_create(primme_amd_svds_operator **out, hipk_ctx *ctx, int dt,
      int64_t m, int64_t n, const int32_t *rp, const int32_t *ci, const void *val) {
   primme_amd_svds_operator *op = (primme_amd_svds_operator *)calloc(1, sizeof(*op));
   if (!op) return -2;
   const size_t es = (dt == HIPK_F64) ? 8 : 4;
   int32_t *rpT = NULL, *ciT = NULL;
   void *vT = NULL;
   int rc = hipk_csr_create_rect(ctx, (hipk_dtype)dt, m, n, rp, ci, val, &op->A);
   if (!rc) rc = primme_amd_csr_transpose(m, n, rp, ci, val, es, &rpT, &ciT, &vT);
   if (!rc) rc = hipk_csr_create_rect(ctx, (hipk_dtype)dt, n, m, rpT, ciT, vT, &op->At);
   primme_amd_host_free(rpT); primme_amd_host_free(ciT); primme_amd_host_free(vT);
   if (rc) { if (op->A) hipk_csr_destroy(op->A); free(op); return rc; }
   *out = op;
   return 0;
}
extern "C" int primme_amd_svds_operator_create_dist(primme_amd_svds_operator **out, hipk_ctx *ctx, int dt,
      int64_t mLocal, int64_t n, int64_t nLocal, const int32_t *rp, const int32_t *ci, const void *val, void *comm) {
   primme_amd_comm *c = (primme_amd_comm *)comm;
   if (!c || nLocal * primme_amd_comm_size(c) != n) return -1;     /* equal column slabs */
   int rc = primme_amd_svds_operator_create(out, ctx, dt, mLocal, n, rp, ci, val);
   if (rc) return rc;
   (*out)->comm = c; (*out)->mLocal = mLocal; (*out)->n = n; (*out)->nLocal = nLocal; (*out)->dt = (hipk_dtype)dt;
   return 0;
}

extern "C" int primme_amd_svds_operator_destroy(primme_amd_svds_operator *op) {
   if (!op) return 0;
   if (op->full) (void)hipFree(op->full);
   if (op->jac_r) (void)hipFree(op->jac_r);
   if (op->jac_c) (void)hipFree(op->jac_c);
   for (int i = 0; i < 2; i++) {
      if (op->cheb_p[i]) (void)hipFree(op->cheb_p[i]);
      if (op->cheb_w[i]) (void)hipFree(op->cheb_w[i]);
   }
   hipk_csr_destroy(op->A); hipk_csr_destroy(op->At);
   free(op);
   return 0;
}
/* diag(A A') - shift^2 and diag(A'A) - shift^2 (reference tests/COMMON/mat.c:353-393, the driver's
 * "jacobi" choice for singular value problems); single-rank operators */
extern "C" int primme_amd_svds_operator_set_jacobi(primme_amd_svds_operator *op, const int32_t *rp,
      const int32_t *ci, const void *val, double shift) {
   if (!op || op->comm) return -44;
   const int64_t m = hipk_csr_nrows(op->A), n = hipk_csr_nrows(op->At);
   const hipk_dtype dt = hipk_csr_dtype(op->A);
   const size_t es = (dt == HIPK_F64) ? 8 : 4;
   double *sum = (double *)calloc((size_t)(m + n) + 1, sizeof(double));
   char *packed = (char *)malloc(es * (size_t)(m + n) + 1);
   if (!sum || !packed) { free(sum); free(packed); return -2; }
   for (int64_t i = 0; i < m; i++)
      for (int32_t k = rp[i]; k < rp[i + 1]; k++) {
         const double v = (dt == HIPK_F64) ? ((const double *)val)[k] : (double)((const float *)val)[k];
         sum[i] += v * v;
         sum[m + ci[k]] += v * v;
      }
   for (int64_t i = 0; i < m + n; i++) {
      double d = sum[i] - shift * shift;
      if (fabs(d) < 1e-14) d = copysign(1e-14, d);
      if (dt == HIPK_F64) ((double *)packed)[i] = d; else ((float *)packed)[i] = (float)d;
   }
   free(sum);
   if (!op->jac_r && hipMalloc(&op->jac_r, es * (size_t)(m > 0 ? m : 1)) != hipSuccess) { free(packed); return -2; }
   if (!op->jac_c && hipMalloc(&op->jac_c, es * (size_t)(n > 0 ? n : 1)) != hipSuccess) { free(packed); return -2; }
   /* through pinned staging on the stream the operator's kernels run on (hipk_upload: never the NULL stream) */
   hipk_ctx *octx = hipk_csr_ctx(op->A);
   const int e1 = m > 0 ? hipk_upload(octx, op->jac_r, packed, es * (size_t)m) : 0;
   const int e2 = n > 0 ? hipk_upload(octx, op->jac_c, packed + es * (size_t)m, es * (size_t)n) : 0;
   free(packed);
   return (e1 == 0 && e2 == 0) ? 0 : -1;
}

/* applyPreconditioner of primme_svds_params for the operator's Jacobi data: y = x / diag(A'A),
 * x / diag(AA') or both halves for the augmented operator (mat.c:395-426) */
extern "C" void primme_amd_svds_jacobi_precond(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy, int *blockSize,
      int *mode, struct primme_svds_params *ps, int *ierr) {
   primme_amd_svds_operator *op = (primme_amd_svds_operator *)ps->preconditioner;
   *ierr = 1;
   if (!op || !op->jac_r || !op->jac_c) return;
   void *stream = ps->queue ? (void *)*(hipStream_t *)ps->queue : NULL;
   const hipk_dtype dt = hipk_csr_dtype(op->A);
   const size_t es = (dt == HIPK_F64) ? 8 : 4;
   const double min_den = 1e-14 * (ps->aNorm >= 0.0 ? ps->aNorm : 1.0);
   const int64_t m = ps->mLocal, n = ps->nLocal;
   int rc = 0;
   for (int c0 = 0; c0 < *blockSize && !rc; c0 += 64) {
      const int nb = *blockSize - c0 < 64 ? *blockSize - c0 : 64;
      double zeros[64] = {0};
      const char *xc = (const char *)x + (size_t)c0 * *ldx * es;
      char *yc = (char *)y + (size_t)c0 * *ldy * es;
      if (*mode == primme_svds_op_AtA) rc = hipk_jacobi_apply(stream, dt, n, op->jac_c, zeros, min_den, xc, *ldx, yc, *ldy, nb);
      else if (*mode == primme_svds_op_AAt) rc = hipk_jacobi_apply(stream, dt, m, op->jac_r, zeros, min_den, xc, *ldx, yc, *ldy, nb);
      else if (*mode == primme_svds_op_augmented) {
         rc = hipk_jacobi_apply(stream, dt, n, op->jac_c, zeros, min_den, xc, *ldx, yc, *ldy, nb);
         if (!rc) rc = hipk_jacobi_apply(stream, dt, m, op->jac_r, zeros, min_den, xc + (size_t)n * es, *ldx, yc + (size_t)n * es, *ldy, nb);
      } else rc = 1;
   }
   *ierr = rc ? 1 : 0;
}

/* ---- Chebyshev polynomial preconditioner for the singular value solver ---------------------------------
 * With lo = slo^2, hi = shi^2, sigma = sshift^2 and p the polynomial of primme_amd_chebyshev_precond above (the steps-th
 * Chebyshev iterate for (M - sigma I) y = x from y = 0):
 *    primme_svds_op_AtA        y = p(A'A) x
 *    primme_svds_op_AAt        y = p(AA') x
 *    primme_svds_op_augmented  y = (B + sshift I) diag(p(A'A), p(AA')) x,  B = [0 A'; A 0], x = [v; u]
 * (on an eigenvector of B with eigenvalue l the last one is (1 - q(l^2)) / (l - sshift): symmetric, commutes with B).
 * One step of p(A'A): z = A y_k (plain product), then Out = cy y_k + cp y_{k-1} + cx x + cw A'z — in one pass over A' with
 * hipk_csr_cheb_step_gather (G = z), or A'z into a product panel + hipk_cheb_update.  Widest block for which the one-pass
 * step is the default: where the kernel trace shows it not slower.  It is slower at both widths measured (66.7 against 62.2 us
 * at one column, 381 against 316 us at eight, A' of a 4 M x 3 M band matrix; profiles/svds_cheb_step_kernels.md), so the
 * generic pair is the default; PRIMME_AMD_CHEB_FUSED=1 takes the one-pass step at every width, PRIMME_AMD_CHEB_UNFUSED=1 at none. */
#define CHEB_FUSE_GATHER_MAXCOLS 0

extern "C" int primme_amd_svds_operator_norm_bound(primme_amd_svds_operator *op, double *bound) {
   if (!op || !bound) return -1;
   if (op->comm) return -44;
   double rinf = 0.0, r1 = 0.0;
   int rc = hipk_csr_abs_rowsum_max(op->A, NULL, &rinf);
   if (!rc) rc = hipk_csr_abs_rowsum_max(op->At, NULL, &r1);
   if (rc) return rc;
   *bound = sqrt(rinf * r1);            /* |A|_2^2 <= |A|_1 |A|_inf */
   return 0;
}

extern "C" int primme_amd_svds_operator_set_chebyshev(primme_amd_svds_operator *op, int steps, double slo, double shi, double sshift) {
   if (!op) return -1;
   if (op->comm) return -44;
   if (steps < 1 || slo != slo || slo < 0.0 || sshift != sshift || sshift < 0.0) return -1;    /* singular value units: nothing is negative */
   if (shi != shi && primme_amd_svds_operator_norm_bound(op, &shi)) return -1;
   if (!(slo < shi) || (sshift > slo && sshift < shi)) return -1;
   op->cheb_steps = steps; op->cheb_lo = slo * slo; op->cheb_hi = shi * shi; op->cheb_sigma = sshift * sshift; op->cheb_sshift = sshift;
   const char *e = getenv("PRIMME_AMD_CHEB_UNFUSED");
   op->cheb_unfused = e && atoi(e) != 0;
   e = getenv("PRIMME_AMD_CHEB_FUSED");
   op->cheb_fused_all = e && atoi(e) != 0;
   return 0;
}

/* Out = cx X + cw F G (+ cy Yk + cp Yprev) for nc columns, F = A (rows: m-vectors) or A' : the one-pass kernel when `fuse`
 * and the matrix has the form for it (*fuse is cleared when it has not), else the product into the side's product panel and
 * hipk_cheb_update */
static int svds_cheb_combine(primme_amd_svds_operator *op, void *stream, int side, int *fuse, int nc, const hipk_cheb_coef *cf,
      const void *X, int64_t ldx, const void *G, int64_t ldg, const void *Yk, int64_t ldk, const void *Yp, int64_t ldp, void *Out, int64_t ldo) {
   hipk_csr *Fm = side ? op->A : op->At;
   const hipk_dtype dt = hipk_csr_dtype(op->A);
   g_cheb_products += nc;
   if (*fuse) {
      const int rc = hipk_csr_cheb_step_gather(Fm, stream, nc, cf, X, ldx, G, ldg, Yk, ldk, Yp, ldp, Out, ldo);
      if (rc == 0) g_cheb_fused += nc;
      if (rc != 1) return rc;
      *fuse = 0;
   }
   const size_t es = op_elem(dt);
   if (op->cheb_wcols[side] < op->cheb_cols) {
      if (op->cheb_w[side]) (void)hipFree(op->cheb_w[side]);
      op->cheb_w[side] = NULL; op->cheb_wcols[side] = 0;
      if (hipMalloc(&op->cheb_w[side], (size_t)op->cheb_ld[side] * es * op->cheb_cols) != hipSuccess) return -2;
      op->cheb_wcols[side] = op->cheb_cols;
   }
   int rc = hipk_csr_matvec(Fm, stream, G, ldg, op->cheb_w[side], op->cheb_ld[side], nc);
   if (!rc) rc = hipk_cheb_update(stream, dt, hipk_csr_nrows(Fm), nc, cf, X, ldx, op->cheb_w[side], op->cheb_ld[side], Yk, ldk, Yp, ldp, Out, ldo);
   return rc;
}

/* p(M) x for nc <= HIPK_CHEB_MAXCOLS columns, M = A'A (side 0) or AA' (side 1).  out == NULL: the result stays in the side's
 * panel number steps % 2 (its other panel and the other side's panel number steps % 2 are left alone) */
static int svds_cheb_poly(primme_amd_svds_operator *op, void *stream, int side, int *fuse, int nc, const char *x, int64_t lx, char *out, int64_t ldo) {
   hipk_csr *first = side ? op->At : op->A;
   const hipk_dtype dt = hipk_csr_dtype(op->A);
   const size_t es = op_elem(dt);
   const int d = op->cheb_steps;
   const int64_t ld = op->cheb_ld[side], ldz = op->cheb_ld[!side], rows = hipk_csr_nrows(side ? op->A : op->At);
   char *P[2] = {(char *)op->cheb_p[side], (char *)op->cheb_p[side] + (size_t)ld * es * op->cheb_cols};
   char *z = (char *)op->cheb_p[!side] + (size_t)((d + 1) % 2) * ldz * es * op->cheb_cols;
   const double lo = op->cheb_lo, hi = op->cheb_hi, dl = 0.5 * (hi - lo), sigma = op->cheb_sigma, tb = 0.5 * (hi + lo) - sigma;
   double rho[HIPK_CHEB_MAXCOLS];
   hipk_cheb_coef cf;
   memset(&cf, 0, sizeof(cf));
   for (int c = 0; c < nc; c++) { rho[c] = dl / tb; cf.cx[c] = 1.0 / tb; }
   if (!out) { out = P[d % 2]; ldo = ld; }
   if (d == 1) return hipk_cheb_update(stream, dt, rows, nc, &cf, x, lx, NULL, 0, NULL, 0, NULL, 0, out, ldo);
   for (int k = 1; k < d; k++) {
      for (int c = 0; c < nc; c++) cheb_step_coef(tb, dl, sigma, k, &rho[c], &cf, c);
      /* as in primme_amd_chebyshev_precond: y_1 = x / tb is never stored, y_{k+1} goes over y_{k-1}, the last one to `out` */
      const char *yk = k == 1 ? x : P[k % 2], *yp = k == 1 ? NULL : (k == 2 ? x : P[(k + 1) % 2]);
      const int64_t ldk = k == 1 ? lx : ld, ldp = k == 2 ? lx : ld;
      char *o = k == d - 1 ? out : P[(k + 1) % 2];
      const int64_t lo_ = k == d - 1 ? ldo : ld;
      int rc = hipk_csr_matvec(first, stream, yk, ldk, z, ldz, nc);
      g_cheb_products += nc;
      if (!rc) rc = svds_cheb_combine(op, stream, side, fuse, nc, &cf, x, lx, z, ldz, yk, ldk, yp, ldp, o, lo_);
      if (rc) return rc;
   }
   return 0;
}

extern "C" void primme_amd_svds_chebyshev_precond(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy, int *blockSize,
      int *mode, struct primme_svds_params *ps, int *ierr) {
   primme_amd_svds_operator *op = (primme_amd_svds_operator *)ps->preconditioner;
   *ierr = 1;
   if (!op || op->comm || op->cheb_steps < 1) return;
   if (*mode != primme_svds_op_AtA && *mode != primme_svds_op_AAt && *mode != primme_svds_op_augmented) return;
   if (*blockSize <= 0) { *ierr = 0; return; }
   void *stream = ps->queue ? (void *)*(hipStream_t *)ps->queue : NULL;
   if (!stream) stream = hipk_ctx_stream(hipk_csr_ctx(op->A));
   const hipk_dtype dt = hipk_csr_dtype(op->A);
   const size_t es = op_elem(dt);
   /* vector lengths from the matrices: for the real-equivalent form of a complex matrix they are the 2n / 2m real rows, and the
    * leading dimensions, which arrive in complex elements, double (the recurrence has real coefficients) */
   const int64_t len[2] = {hipk_csr_nrows(op->At), hipk_csr_nrows(op->A)};
   const int64_t f = op->cplx ? 2 : 1, lx = f * *ldx, ly = f * *ldy;
   const int d = op->cheb_steps;
   const int want = *blockSize < HIPK_CHEB_MAXCOLS ? *blockSize : HIPK_CHEB_MAXCOLS;
   if (want > op->cheb_cols) {
      for (int i = 0; i < 2; i++) {
         if (op->cheb_p[i]) (void)hipFree(op->cheb_p[i]);
         if (op->cheb_w[i]) (void)hipFree(op->cheb_w[i]);
         op->cheb_p[i] = op->cheb_w[i] = NULL; op->cheb_wcols[i] = 0;
      }
      op->cheb_cols = 0;
      for (int i = 0; i < 2; i++) {
         op->cheb_ld[i] = (len[i] + 3) / 4 * 4 + 4;           /* columns on 16-byte boundaries */
         if (hipMalloc(&op->cheb_p[i], (size_t)op->cheb_ld[i] * es * 2 * want) != hipSuccess) return;
      }
      op->cheb_cols = want;
   }
   int fuse = !op->cheb_unfused;
   int rc = 0;
   for (int c0 = 0; c0 < *blockSize && !rc; c0 += HIPK_CHEB_MAXCOLS) {
      const int nc = *blockSize - c0 < HIPK_CHEB_MAXCOLS ? *blockSize - c0 : HIPK_CHEB_MAXCOLS;
      const char *xc = (const char *)x + (size_t)c0 * lx * es;
      char *yc = (char *)y + (size_t)c0 * ly * es;
      int fz = fuse && (op->cheb_fused_all || nc <= CHEB_FUSE_GATHER_MAXCOLS);
      g_cheb_applies += nc;
      if (*mode != primme_svds_op_augmented) {
         rc = svds_cheb_poly(op, stream, *mode == primme_svds_op_AAt, &fz, nc, xc, lx, yc, ly);
      } else {
         /* t_v = p(A'A) v and t_u = p(AA') u into panel d % 2 of either side, then [y_v; y_u] = [sshift t_v + A' t_u; sshift t_u + A t_v] */
         const size_t uoff = (size_t)len[0] * es;
         rc = svds_cheb_poly(op, stream, 0, &fz, nc, xc, lx, NULL, 0);
         if (!rc) rc = svds_cheb_poly(op, stream, 1, &fz, nc, xc + uoff, lx, NULL, 0);
         const char *tv = (const char *)op->cheb_p[0] + (size_t)(d % 2) * op->cheb_ld[0] * es * op->cheb_cols;
         const char *tu = (const char *)op->cheb_p[1] + (size_t)(d % 2) * op->cheb_ld[1] * es * op->cheb_cols;
         hipk_cheb_coef cf;
         memset(&cf, 0, sizeof(cf));
         for (int c = 0; c < nc; c++) { cf.cx[c] = op->cheb_sshift; cf.cw[c] = 1.0; }
         if (!rc) rc = svds_cheb_combine(op, stream, 0, &fz, nc, &cf, tv, op->cheb_ld[0], tu, op->cheb_ld[1], NULL, 0, NULL, 0, yc, ly);
         if (!rc) rc = svds_cheb_combine(op, stream, 1, &fz, nc, &cf, tu, op->cheb_ld[1], tv, op->cheb_ld[0], NULL, 0, NULL, 0, yc + uoff, ly);
      }
      if (fuse && (op->cheb_fused_all || nc <= CHEB_FUSE_GATHER_MAXCOLS) && !fz) fuse = 0;   /* no one-pass form for these matrices */
   }
   *ierr = rc ? 1 : 0;
}

extern "C" int primme_amd_svds_operator_is_local(const void *op) { return op && ((const primme_amd_svds_operator *)op)->comm == NULL; }

extern "C" int primme_amd_svds_operator_set_complex(primme_amd_svds_operator *op, int on) {
   if (!op) return -1;
   op->cplx = on ? 1 : 0;
   return 0;
}

extern "C" void primme_amd_svds_matvec(void *x, PRIMME_INT *ldx, void *y, PRIMME_INT *ldy, int *blockSize,
      int *transpose, struct primme_svds_params *ps, int *ierr) {
   primme_amd_svds_operator *op = (primme_amd_svds_operator *)ps->matrix;
   void *stream = ps->queue ? (void *)*(hipStream_t *)ps->queue : NULL;
   *ierr = 1;
   if (!op) return;
   if (!op->comm) {
      const int64_t f = op->cplx ? 2 : 1;
      *ierr = hipk_csr_matvec(*transpose ? op->At : op->A, stream, x, f * *ldx, y, f * *ldy, *blockSize);
      return;
   }
   if (op->cplx) return;
   /* row-partitioned A: the block goes through the [n x blockSize] staging panel with ONE grouped
    * collective (a column per call inside an RCCL group) and ONE SpMM per application */
   const size_t es = (op->dt == HIPK_F64) ? 8 : 4;
   const int nb = *blockSize;
   if (nb <= 0) { *ierr = 0; return; }
   if (grow(&op->full, &op->full_cap, (size_t)op->n * nb * es)) return;
   if (!*transpose) {
      if (primme_amd_comm_allgather_cols(op->comm, stream, x, *ldx, op->full, op->n, (size_t)op->nLocal * es, es, nb)) return;
      if (hipk_csr_matvec(op->A, stream, op->full, op->n, y, *ldy, nb)) return;
   } else {
      if (hipk_csr_matvec(op->At, stream, x, *ldx, op->full, op->n, nb)) return;
      if (primme_amd_comm_reduce_scatter_cols(op->comm, stream, op->full, op->n, y, *ldy, (size_t)op->nLocal, op->dt == HIPK_F64, nb)) return;
   }
   *ierr = 0;
}
