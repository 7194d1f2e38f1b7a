/* hipk_csr.hip — the hipk_csr object: the user's matrix on the device.  Creation (the host analysis is
 * primme_amd_csr_tile_plan of csr_tools.c; the other forms are built by their own units), the queries, the ROUTING of every
 * product to the form and kernel that serve it (csr_route_of), and the public products.  The row-tile and stencil kernels
 * and their launchers are in hipk_sparse.hip, the panel-blocked / row-pattern / sliced-ELL forms in hipk_sparse_{pb,pat,sell}.hip.
 */
#include "hipk_sparse_dev.h"

const csr_knob_set &csr_knobs(void) {
   static csr_knob_set K;
   static bool read = false;
   if (!read) {
      const char *e;
      K.nc = (e = getenv("HIPK_SPMM_NC")) ? atoi(e) : 0;
      K.no_window = getenv("HIPK_NO_WINDOW") != NULL;
      K.no_split = getenv("HIPK_SPMM_NO_SPLIT") != NULL;
      K.even_stride = getenv("HIPK_SPMM_EVEN_STRIDE") != NULL;
      K.big_window = getenv("HIPK_SPMM_BIG_WINDOW") != NULL;
      K.no_col16 = getenv("HIPK_SPMM_NO_COL16") != NULL;
      K.nt = (e = getenv("HIPK_SPMV_NT")) ? atoi(e) : -1;
      K.pb_maxcols = (e = getenv("HIPK_PB_MAXCOLS")) ? atoi(e) : 2;
      read = true;
   }
   return K;
}

/* THE routing decision: every entry point and query below calls it and switches on the record; a new form or kernel is
 * added here and nowhere else.
 *   own   pat, sell and pb exclude one another at creation; hipk_set_spmv_format(0) switches pat and sell off
 *   form  the plain product goes to sell (any width), pat (one column) or pb (up to HIPK_PB_MAXCOLS columns); the shifted
 *         one to sell; the Chebyshev step and the fused-scaled product to pat; the gather step to nothing but the row tiles
 *         (its caller declines when `own` is another form); everything else falls to the row tiles
 *   row tiles  the windowed kernel for every product with an epilogue (shift, Chebyshev) and for blocks of a windowed matrix,
 *         the stream kernel for one column, the plain row-block kernel for the rest */
csr_route csr_route_of(const hipk_csr *A, int ncols, int op) {
   const csr_knob_set &K = csr_knobs();
   csr_route r;
   memset(&r, 0, sizeof r);
   const double es = (double)hipk_elem_size(A->dt);
   const double vec = (op == CSR_OP_SCALED ? 3.0 : 2.0) * A->nrows * es * ncols;
   r.index_bytes = 4;
   if (A->kind == 1) {
      r.own = r.form = CSR_STENCIL;
      r.alg = r.streamed = vec;
      return r;
   }
   const bool on = hipk_pat_enabled() != 0;
   r.own = (A->pat && on) ? CSR_PAT : (A->sell && on) ? CSR_SELL : A->pb ? CSR_PB : CSR_TILES;
   const bool plain = op == CSR_OP_PLAIN, epilogue = op == CSR_OP_SHIFTED || op == CSR_OP_CHEB || op == CSR_OP_CHEB_GATHER;
   const bool serves = r.own == CSR_SELL ? (plain || op == CSR_OP_SHIFTED)
                     : r.own == CSR_PAT  ? ((plain && ncols == 1) || op == CSR_OP_CHEB || op == CSR_OP_SCALED)
                     : r.own == CSR_PB   ? (plain && ncols <= K.pb_maxcols)
                     : true;
   r.form = (serves || op == CSR_OP_CHEB_GATHER) ? r.own : CSR_TILES;

   r.c16 = A->col16 && !K.no_col16;
   if (op != CSR_OP_SCALED && A->halo_lo == 0 && A->halo_hi == 0 && ncols <= 64 && ((A->windowed && ncols >= 2 && !K.no_window) || epilogue)) {
      r.kernel = CSR_K_WINDOW;
      r.nc = ncols <= 2 ? 2 : 4;
      r.xs_small = !K.big_window && (int64_t)A->cw_max * (K.even_stride ? ncols : (ncols | 1)) <= XS_SMALL;
   } else if (op == CSR_OP_SCALED || (ncols == 1 && K.nc == 0)) {
      r.kernel = CSR_K_STREAM;
   } else {
      r.kernel = CSR_K_ROWS;
      r.nc = K.nc == 1 ? 1 : (K.nc == 2 || (K.nc == 0 && ncols <= 2)) ? 2 : 4;
      r.c16 = 0;                                   /* this kernel reads the 4-byte columns */
   }
   if (r.c16) r.index_bytes = 2;
   /* stream the matrix past the Infinity Cache?  Yes when its (value, index) stream alone is more than about three quarters
    * of the 256 MiB (it cannot stay until the next product anyway) */
   r.nt = r.kernel == CSR_K_STREAM && (K.nt >= 0 ? K.nt != 0 : (double)A->nnz * (es + r.index_bytes) > 192.0 * 1024 * 1024);

   r.alg = (double)A->nnz * (es + 4) + (A->nrows + 1) * 4.0 + vec;
   switch (r.form) {
   case CSR_SELL: r.streamed = hipk_sell_bytes(A->sell, ncols); break;
   case CSR_PAT: r.streamed = hipk_pat_bytes(A->pat, op == CSR_OP_SCALED); break;
   case CSR_PB: r.streamed = hipk_pb_bytes(A->pb) * ncols; break;
   default:
      r.streamed = (double)A->nnz * (es + r.index_bytes) + (A->nrows + 1) * 4.0 + vec;
      /* (the fused product of a matrix held in panel-blocked form has always been accounted as that form's product plus
       * the second output, though the stream kernel serves it) */
      if (op == CSR_OP_SCALED && r.own == CSR_PB) r.streamed = hipk_pb_bytes(A->pb) + (double)A->nrows * es;
   }
   return r;
}

/* Validation, the host analysis, allocation and upload, then the builders of the other forms.  One failure path: whatever
 * the partly built handle holds goes through hipk_csr_destroy. */
static int csr_create_impl(hipk_ctx *ctx, hipk_dtype dt, int64_t nrows_local,
      int64_t ncols_global, int64_t row0, int64_t x0, int64_t xlen, const int32_t *rowptr_host,
      const int32_t *colind_host, const void *values_host, unsigned flags, hipk_csr **out) {
   if (dt != HIPK_F64 && dt != HIPK_F32 && dt != HIPK_C64 && dt != HIPK_C32) return -44;
   if (nrows_local >= ((int64_t)1 << 31)) return -1;
   hipk_csr *A = (hipk_csr *)calloc(1, sizeof(hipk_csr));
   if (!A) return -2;
   A->ctx = ctx; A->dt = dt; A->kind = 0;
   A->nrows = nrows_local; A->ncols_global = ncols_global; A->row0 = row0;
   A->x0 = x0; A->xlen = xlen;
   const int64_t nnz = rowptr_host[nrows_local];
   A->nnz = nnz;
   const size_t es = hipk_elem_size(dt);
   const bool real = dt == HIPK_F64 || dt == HIPK_F32;
   primme_amd_tile_plan *P = NULL;
   int rc = primme_amd_csr_tile_plan(nrows_local, row0, x0, xlen, ncols_global, rowptr_host, colind_host, values_host, es, real, &P) ? -2 : 0;
   if (!rc) {
      A->halo_lo = A->ld_lo = P->halo_lo; A->halo_hi = A->ld_hi = P->halo_hi;
      A->ntiles = P->ntiles; A->cw_max = P->cw_max; A->windowed = P->windowed;
      A->c16back = P->col16 ? P->c16back : 0;
      const size_t nt1 = (size_t)P->ntiles + 1;
      if (hipk_malloc(ctx, (size_t)(nrows_local + 1) * 4, (void **)&A->rowptr) ||
            hipk_malloc(ctx, (size_t)(nnz + 1) * 4, (void **)&A->colind) ||       /* +1: clamped loads of an empty tile */
            hipk_malloc(ctx, (size_t)(nnz + 1) * es, &A->values) ||
            hipk_malloc(ctx, nt1 * 4, (void **)&A->tiles) ||
            hipk_malloc(ctx, nt1 * sizeof(int4), (void **)&A->tileinfo) ||
            hipk_malloc(ctx, nt1 * sizeof(int2), (void **)&A->twin) ||
            hipk_malloc(ctx, (size_t)nrows_local * es, &A->diag) ||
            (P->col16 && hipk_malloc(ctx, (size_t)(nnz + 1) * sizeof(uint16_t), (void **)&A->col16)))
         rc = -2;
   }
   /* Every upload goes through pinned staging on the context's stream (hipk_upload) and is complete on return: nothing
    * goes through the NULL stream, which a hipStreamNonBlocking stream is not ordered against, and the runtime is never
    * asked to copy asynchronously out of the caller's pageable arrays. */
   if (!rc) {
      /* the padded element behind the last nonzero (clamped loads of trailing empty tiles): value 0 and a column
       * inside the owned slab, so that the gather stays in range with halos too */
      const int32_t padcol = (int32_t)x0;
      const char zero[16] = {0};
      const size_t nt1 = (size_t)P->ntiles + 1;
      if (hipk_upload(ctx, A->rowptr, rowptr_host, (size_t)(nrows_local + 1) * 4) ||
            hipk_upload(ctx, A->colind, colind_host, (size_t)nnz * 4) ||
            hipk_upload(ctx, A->values, values_host, (size_t)nnz * es) ||
            hipk_upload(ctx, A->tiles, P->tiles, nt1 * 4) ||
            hipk_upload(ctx, A->tileinfo, P->info, nt1 * sizeof(int4)) ||
            hipk_upload(ctx, A->twin, P->win, nt1 * sizeof(int2)) ||
            hipk_upload(ctx, A->diag, P->diag, (size_t)nrows_local * es) ||
            (A->col16 && hipk_upload(ctx, A->col16, P->col16, (size_t)(nnz + 1) * sizeof(uint16_t))) ||
            hipk_upload(ctx, A->colind + nnz, &padcol, (size_t)4) ||
            hipk_upload(ctx, (char *)A->values + (size_t)nnz * es, zero, es))
         rc = -1;
   }
   primme_amd_tile_plan_free(P);
   const bool local = A->halo_lo == 0 && A->halo_hi == 0;
   /* scattered column pattern over an input vector that is all local (the rectangular operators of the singular value
    * problem): the panel-blocked form serves the one-column products */
   if (!rc && local && x0 == 0 && xlen == ncols_global && real) {
      const int rcp = hipk_pb_build(ctx, dt, nrows_local, ncols_global, rowptr_host, colind_host, values_host, &A->pb);
      if (rcp < 0) rc = rcp;
   }
   /* rows that repeat (constant-coefficient stencils, lattice operators): one byte per row + a pattern table serves the
    * one-column products (hipk_sparse_pat.hip); the offsets are taken against the row, so the input entries must be
    * numbered like the rows AND be as many as the rows (square operators, row slabs with halos): pat_kernel sizes its x
    * descriptor, its end-of-vector test and the own-row reads of its padded table entries from nrows, so a rectangular
    * operator (hipk_csr_create_rect: x0 == row0 == 0 but xlen != nrows — A and A' of the singular value problem when the
    * panel-blocked builder declines) must stay on the row tiles */
   if (!rc && x0 == row0 && xlen == nrows_local && real && !A->pb) {
      const int rcp = hipk_pat_build(ctx, dt, nrows_local, row0, rowptr_host, colind_host, values_host, &A->pat);
      if (rcp < 0) rc = rcp;
      /* HIPK_CSR_DIAG_PATTERNS: the exact scan gave up — rows that repeat but for their diagonal entry (stencil / lattice
       * operator + potential) take the diagonal-split flavour, which streams A->diag beside the pattern bytes */
      if (!rc && !A->pat && (flags & HIPK_CSR_DIAG_PATTERNS)) {
         const int rcd = hipk_pat_build_diag(ctx, dt, nrows_local, row0, rowptr_host, colind_host, values_host, A->diag, &A->pat);
         if (rcd < 0) rc = rcd;
      }
   }
   /* HIPK_CSR_SLICED: a general matrix (neither of the forms above took it) whose rows and input entries coincide and are
    * all local also gets the sliced-ELL form, when its padding stays within 1.25 nnz (hipk_sparse_sell.hip); anything
    * else keeps the row tiles alone */
   if (!rc && (flags & HIPK_CSR_SLICED) && real && local && x0 == row0 && xlen == nrows_local &&
         ncols_global >= row0 + nrows_local && !A->pb && !A->pat) {
      const int rcs = hipk_sell_build(ctx, dt, nrows_local, rowptr_host, colind_host, values_host, &A->sell);
      if (rcs < 0) rc = rcs;
   }
   if (rc) { hipk_csr_destroy(A); return rc; }
   *out = A;
   return 0;
}

extern "C" int hipk_csr_create_opts(hipk_ctx *ctx, hipk_dtype dt, int64_t nrows_local,
      int64_t ncols_global, int64_t row0, const int32_t *rowptr_host,
      const int32_t *colind_host, const void *values_host, unsigned flags, hipk_csr **out) {
   return csr_create_impl(ctx, dt, nrows_local, ncols_global, row0, row0, nrows_local, rowptr_host,
         colind_host, values_host, flags, out);
}
/* the flags of hipk_csr_create: HIPK_SPMV_PAT_DIAG=1 in the environment asks for the diagonal-split row patterns,
 * HIPK_SPMV_SELL=1 for the sliced-ELL form (default: none) */
extern "C" int hipk_csr_create(hipk_ctx *ctx, hipk_dtype dt, int64_t nrows_local,
      int64_t ncols_global, int64_t row0, const int32_t *rowptr_host,
      const int32_t *colind_host, const void *values_host, hipk_csr **out) {
   const char *e = getenv("HIPK_SPMV_PAT_DIAG"), *s = getenv("HIPK_SPMV_SELL");
   return hipk_csr_create_opts(ctx, dt, nrows_local, ncols_global, row0, rowptr_host, colind_host, values_host,
         ((e && atoi(e) != 0) ? HIPK_CSR_DIAG_PATTERNS : 0u) | ((s && atoi(s) != 0) ? HIPK_CSR_SLICED : 0u), out);
}
extern "C" int hipk_csr_create_rect(hipk_ctx *ctx, hipk_dtype dt, int64_t nrows, int64_t ncols,
      const int32_t *rowptr_host, const int32_t *colind_host, const void *values_host, hipk_csr **out) {
   return csr_create_impl(ctx, dt, nrows, ncols, 0, 0, ncols, rowptr_host, colind_host, values_host, 0u, out);
}

extern "C" int hipk_stencil_create(hipk_ctx *ctx, hipk_dtype dt, int nx, int ny, int nz,
      int64_t row0, int64_t nrows_local, hipk_csr **out) {
   if (dt != HIPK_F64 && dt != HIPK_F32) return -44;
   hipk_csr *A = (hipk_csr *)calloc(1, sizeof(hipk_csr));
   if (!A) return -2;
   A->ctx = ctx; A->dt = dt; A->kind = 1;
   A->sx = nx; A->sy = ny > 0 ? ny : 1; A->sz = nz > 0 ? nz : 1;
   const int64_t n = (int64_t)A->sx * A->sy * A->sz;
   A->nrows = nrows_local; A->ncols_global = n; A->row0 = row0;
   A->x0 = row0; A->xlen = nrows_local;
   const int dims = (A->sz > 1) ? 3 : (A->sy > 1 ? 2 : 1);
   A->nnz = n * (2 * dims + 1); /* nominal */
   /* reach of the stencil outside the slab: one x-y plane (3-D), one x line (2-D) */
   const int64_t reach = (A->sz > 1) ? (int64_t)A->sx * A->sy : (A->sy > 1 ? A->sx : 1);
   A->halo_lo = row0 > 0 ? (reach < row0 ? reach : row0) : 0;
   const int64_t above = n - (row0 + nrows_local);
   A->halo_hi = above > 0 ? (reach < above ? reach : above) : 0;
   A->ld_lo = A->halo_lo; A->ld_hi = A->halo_hi;
   const int rc = hipk_malloc(ctx, (size_t)nrows_local * hipk_elem_size(dt), &A->diag) ? -2 : hipk_fill(ctx, dt, A->diag, nrows_local, 2.0 * dims);
   if (rc) { hipk_csr_destroy(A); return rc; }
   *out = A;
   return 0;
}

extern "C" int hipk_csr_destroy(hipk_csr *A) {
   if (!A) return 0;
   hipStreamSynchronize(A->ctx->stream);
   if (A->rowptr) (void)hipFree(A->rowptr);
   if (A->colind) (void)hipFree(A->colind);
   if (A->values) (void)hipFree(A->values);
   if (A->tiles) (void)hipFree(A->tiles);
   if (A->tileinfo) (void)hipFree(A->tileinfo);
   if (A->twin) (void)hipFree(A->twin);
   if (A->col16) (void)hipFree(A->col16);
   if (A->diag) (void)hipFree(A->diag);
   if (A->pb) hipk_pb_destroy(A->pb);
   if (A->pat) hipk_pat_destroy(A->pat);
   if (A->sell) hipk_sell_destroy(A->sell);
   free(A);
   return 0;
}

extern "C" const void *hipk_csr_diag(hipk_csr *A) { return A->diag; }
extern "C" int64_t hipk_csr_nnz(const hipk_csr *A) { return A->nnz; }
extern "C" int64_t hipk_csr_halo_lo(const hipk_csr *A) { return A->halo_lo; }
extern "C" int64_t hipk_csr_halo_hi(const hipk_csr *A) { return A->halo_hi; }
extern "C" int hipk_csr_set_halo(hipk_csr *A, const void *lo, const void *hi) {
   A->xlo = lo; A->xhi = hi; A->ld_lo = A->halo_lo; A->ld_hi = A->halo_hi;
   return 0;
}
extern "C" int hipk_csr_set_halo_ld(hipk_csr *A, const void *lo, int64_t ld_lo, const void *hi, int64_t ld_hi) {
   A->xlo = lo; A->xhi = hi; A->ld_lo = ld_lo; A->ld_hi = ld_hi;
   return 0;
}
extern "C" int hipk_csr_kind(const hipk_csr *A) { return A->kind; }
hipk_ctx *hipk_csr_ctx(const hipk_csr *A) { return A->ctx; }
int hipk_csr_fusable(const hipk_csr *A) { return A && A->kind == 0 && A->x0 == A->row0 && A->xlen == A->nrows && !HIPK_IS_Z(A->dt); }      /* library-internal (hipk_internal.h) */
extern "C" hipk_dtype hipk_csr_dtype(const hipk_csr *A) { return A->dt; }
extern "C" int64_t hipk_csr_nrows(const hipk_csr *A) { return A->nrows; }

/* ---- queries about the form in use: all of them read the route of the one-column product ---- */
/* bytes per nonzero the tile kernels really stream for the index: 2 with the 16-bit index stream, else 4 */
extern "C" int hipk_csr_index_bytes(const hipk_csr *A) { return A ? csr_route_of(A, 1, CSR_OP_PLAIN).index_bytes : 4; }
/* the form that serves the ONE-column products of this matrix right now: 0 CSR row tiles, 1 panel-blocked, 2 row patterns, 3 stencil,
 * 4 sliced ELL */
extern "C" int hipk_csr_format(const hipk_csr *A) { return A ? csr_route_of(A, 1, CSR_OP_PLAIN).own : -1; }
/* bytes ONE one-column product (fused = with the second output of hipk_csr_matvec_scaled) moves through HBM in the form in use */
extern "C" double hipk_csr_product_bytes(const hipk_csr *A, int fused) {
   return A ? csr_route_of(A, 1, fused ? CSR_OP_SCALED : CSR_OP_PLAIN).streamed : 0.0;
}
extern "C" double hipk_csr_streamed_bytes(const hipk_csr *A) {
   if (!A) return 0.0;
   const csr_route rt = csr_route_of(A, 1, CSR_OP_PLAIN);
   return rt.own == CSR_SELL ? rt.streamed : rt.own == CSR_PB ? hipk_pb_bytes(A->pb) : 0.0;
}
/* 1 when the form in use is the row-pattern form in its diagonal-split flavour (the product streams the diagonal) */
extern "C" int hipk_csr_pattern_diag(const hipk_csr *A) { return hipk_csr_format(A) == CSR_PAT && hipk_pat_diag(A->pat); }
/* what was built, whether or not it is switched on right now: panels of the panel-blocked form (0: none), the sliced-ELL form
 * and its padded entries / nnz, the patterns of the row-pattern form */
extern "C" int hipk_csr_panels(const hipk_csr *A) { return A && A->pb ? hipk_pb_panels(A->pb) : 0; }
extern "C" int hipk_csr_sliced(const hipk_csr *A) { return A && A->sell ? 1 : 0; }
extern "C" double hipk_csr_sliced_padding(const hipk_csr *A) { return A && A->sell ? hipk_sell_padding(A->sell) : 0.0; }
extern "C" int hipk_csr_npatterns(const hipk_csr *A) { return A && A->pat ? hipk_pat_npatterns(A->pat) : 0; }

static int csr_halo_missing(const hipk_csr *A) {
   if ((A->halo_lo > 0 && !A->xlo) || (A->halo_hi > 0 && !A->xhi)) {
      fprintf(stderr, "primme_amd: matvec needs halo data (rows outside the local slab) but none was set\n");
      return 1;
   }
   return 0;
}

/* the plain, shifted and Chebyshev-step products of a real matrix, in the form the route names */
template <typename T>
static int csr_matvec_t(hipk_csr *A, int op, hipStream_t stream, const T *x, int64_t ldx, T *y, int64_t ldy, int ncols,
      const double *shift_host = NULL, const SpmmCheb<T> *cheb = NULL) {
   if (csr_halo_missing(A)) return -1;
   const csr_route rt = csr_route_of(A, ncols, op);
   /* the epilogue's other panels */
   const double extra = cheb ? ((cheb->yp ? 2.0 : 1.0) + (cheb->yk && cheb->yk != x ? 1.0 : 0.0)) * A->nrows * sizeof(T) * ncols : 0.0;
   const int pslot = hipk_prof_begin_s(HIPK_PROF_SPMV, stream, cheb ? rt.streamed + extra : rt.alg, rt.streamed + extra);
   int rc = 0;
   switch (rt.form) {
   case CSR_SELL: rc = hipk_sell_matvec(A->sell, stream, A->row0, x, ldx, y, ldy, ncols, shift_host); break;
   case CSR_PAT:
      rc = hipk_pat_matvec(A->pat, stream, hipk_pat_grid(A->pat, A->ctx->num_cu), x, y, A->halo_lo, A->halo_hi, A->xlo, A->xhi, NULL, 0, NULL, NULL, NULL);
      break;
   case CSR_PB: rc = hipk_pb_matvec(A->pb, stream, x, ldx, y, ldy, ncols); break;
   case CSR_STENCIL: csr_launch_stencil<T>(A, stream, x, ldx, y, ldy, ncols); break;
   default: csr_launch_tiles<T>(A, rt, stream, x, ldx, y, ldy, ncols, shift_host, cheb);
   }
   hipk_prof_end(pslot, stream);
   if (rt.form == CSR_STENCIL || rt.form == CSR_TILES) HIPK_CHECK(hipGetLastError());
   return rc;
}

/* complex matrices: the row-tile kernel of hipk_complex.hip (blocks of up to 64 columns per launch) */
static int csr_matvec_z(hipk_csr *A, hipStream_t st, const void *x, int64_t ldx, void *y, int64_t ldy, int ncols, const double *shift_host) {
   if (A->kind != 0) return -44;
   if (csr_halo_missing(A)) return -1;
   const size_t es = hipk_elem_size(A->dt);
   const int pslot = hipk_prof_begin(HIPK_PROF_SPMV, st, csr_route_of(A, ncols, CSR_OP_PLAIN).alg);
   int rc = 0;
   for (int c0 = 0; c0 < ncols && !rc; c0 += 64) {
      const int nc = ncols - c0 < 64 ? ncols - c0 : 64;
      rc = hipk_z_csr_matvec(A->dt, st, A->tileinfo, A->ntiles, A->rowptr, A->colind, A->values, (const char *)x + (size_t)c0 * ldx * es, ldx,
            (char *)y + (size_t)c0 * ldy * es, ldy, nc, A->x0, A->xlen, A->halo_lo, A->halo_hi,
            A->xlo ? (const char *)A->xlo + (size_t)c0 * A->ld_lo * es : NULL, A->xhi ? (const char *)A->xhi + (size_t)c0 * A->ld_hi * es : NULL,
            A->ld_lo, A->ld_hi, shift_host ? shift_host + c0 : NULL);
   }
   hipk_prof_end(pslot, st);
   return rc;
}

extern "C" int hipk_csr_matvec(hipk_csr *A, void *hip_stream, const void *x, int64_t ldx, void *y,
      int64_t ldy, int ncols) {
   if (ncols <= 0 || A->nrows == 0) return 0;
   hipStream_t st = hip_stream ? (hipStream_t)hip_stream : A->ctx->stream;
   if (HIPK_IS_Z(A->dt)) return csr_matvec_z(A, st, x, ldx, y, ldy, ncols, NULL);
   if (A->dt == HIPK_F64) return csr_matvec_t<double>(A, CSR_OP_PLAIN, st, (const double *)x, ldx, (double *)y, ldy, ncols);
   return csr_matvec_t<float>(A, CSR_OP_PLAIN, st, (const float *)x, ldx, (float *)y, ldy, ncols);
}

/* y = A x - shift[c] x(:,c) in one launch (square CSR operators without halo; returns 1 when the
 * operator is not covered and the caller should apply the shift itself) */
extern "C" int hipk_csr_matvec_shifted(hipk_csr *A, void *hip_stream, const void *x, int64_t ldx, void *y, int64_t ldy,
      int ncols, const double *shift_host) {
   if (ncols <= 0 || A->nrows == 0) return 0;
   if (A->kind != 0 || A->halo_lo != 0 || A->halo_hi != 0 || A->x0 != A->row0 || A->xlen != A->nrows || ncols > 64 || !shift_host) return 1;
   hipStream_t st = hip_stream ? (hipStream_t)hip_stream : A->ctx->stream;
   if (HIPK_IS_Z(A->dt)) return csr_matvec_z(A, st, x, ldx, y, ldy, ncols, shift_host);
   if (A->dt == HIPK_F64) return csr_matvec_t<double>(A, CSR_OP_SHIFTED, st, (const double *)x, ldx, (double *)y, ldy, ncols, shift_host);
   return csr_matvec_t<float>(A, CSR_OP_SHIFTED, st, (const float *)x, ldx, (float *)y, ldy, ncols, shift_host);
}

/* the Chebyshev step through csr_matvec_t: G is the gathered panel, the epilogue reads X, Yk, Yprev */
static int csr_cheb_tiles(hipk_csr *A, int op, hipStream_t st, int nx, const hipk_cheb_coef *coef, const void *X, int64_t ldx, const void *G, int64_t ldg,
      const void *Yk, int64_t ldk, const void *Yprev, int64_t ldp, void *Out, int64_t ldo, int seq) {
   if (A->dt == HIPK_F64) {
      const SpmmCheb<double> ep = {*coef, (const double *)X, ldx, (const double *)Yprev, ldp, (const double *)Yk, ldk, seq};
      return csr_matvec_t<double>(A, op, st, (const double *)G, ldg, (double *)Out, ldo, nx, NULL, &ep);
   }
   const SpmmCheb<float> ep = {*coef, (const float *)X, ldx, (const float *)Yprev, ldp, (const float *)Yk, ldk, seq};
   return csr_matvec_t<float>(A, op, st, (const float *)G, ldg, (float *)Out, ldo, nx, NULL, &ep);
}

/* One step of the Chebyshev recurrence with the product inside (include/primme_amd_kernels.h, hipk_cheb.hip):
 * Out = cy Yk + cp Yprev + cx X + cw A Yk.  The row-pattern form runs a column per launch (its kernel owns one column), the
 * row-tile form all columns in one launch of the windowed block kernel.  Same conditions as hipk_csr_matvec_shifted, real
 * matrices only; 1 = not covered. */
extern "C" int hipk_csr_cheb_step(hipk_csr *A, void *hip_stream, int nx, const hipk_cheb_coef *coef, const void *X, int64_t ldx,
      const void *Yk, int64_t ldk, const void *Yprev, int64_t ldp, void *Out, int64_t ldo) {
   if (!A || A->kind != 0 || A->halo_lo != 0 || A->halo_hi != 0 || A->x0 != A->row0 || A->xlen != A->nrows || HIPK_IS_Z(A->dt)) return 1;
   if (nx <= 0 || A->nrows == 0) return 0;
   if (nx > HIPK_CHEB_MAXCOLS || !coef || !X || !Yk || !Out || Out == Yk) return -1;
   hipStream_t st = hip_stream ? (hipStream_t)hip_stream : A->ctx->stream;
   const csr_route rt = csr_route_of(A, 1, CSR_OP_CHEB);
   if (rt.form != CSR_PAT) return csr_cheb_tiles(A, CSR_OP_CHEB, st, nx, coef, X, ldx, Yk, ldk, Yk, ldk, Yprev, ldp, Out, ldo, 0);
   const size_t es = hipk_elem_size(A->dt);
   const int gx = hipk_pat_grid_kind(A->pat, A->ctx->num_cu, 2);
   const double bytes = rt.streamed + (Yprev ? 2.0 : 1.0) * A->nrows * es;
   for (int c = 0; c < nx; c++) {
      const double cf[4] = {coef->cy[c], coef->cp[c], coef->cx[c], coef->cw[c]};
      const int pslot = hipk_prof_begin_s(HIPK_PROF_SPMV, st, bytes, bytes);
      const int rc = hipk_pat_cheb_step(A->pat, st, gx, cf, (const char *)X + (size_t)c * ldx * es, (const char *)Yk + (size_t)c * ldk * es,
            Yprev ? (const char *)Yprev + (size_t)c * ldp * es : NULL, (char *)Out + (size_t)c * ldo * es);
      hipk_prof_end(pslot, st);
      if (rc) return rc;
   }
   return 0;
}

/* The same step for a RECTANGULAR operator (include/primme_amd_kernels.h): Out = cy Yk + cp Yprev + cx X + cw A G, G the only
 * gathered panel (ncols(A) rows), everything else row-local.  One launch of the windowed block kernel for all columns.  The row
 * sum is formed as hipk_csr_matvec forms it for the same matrix and width, so that in double the step equals that product
 * followed by hipk_cheb_update bit for bit: one column: csr_stream_kernel's rounded products (seq = 1); more columns:
 * this very kernel when the matrix is windowed, else csr_rows_block_kernel's fma chain without the two-lane split (seq = -1).
 * 1 = no row-tile form (panel-blocked, row patterns, stencil, halo, complex): the caller runs the generic pair. */
extern "C" int hipk_csr_cheb_step_gather(hipk_csr *A, void *hip_stream, int nx, const hipk_cheb_coef *coef, const void *X, int64_t ldx,
      const void *G, int64_t ldg, const void *Yk, int64_t ldk, const void *Yprev, int64_t ldp, void *Out, int64_t ldo) {
   if (!A) return -1;
   if (csr_route_of(A, nx > 0 ? nx : 1, CSR_OP_CHEB_GATHER).form != CSR_TILES || A->halo_lo != 0 || A->halo_hi != 0 || HIPK_IS_Z(A->dt)) return 1;
   if (nx <= 0 || A->nrows == 0) return 0;
   if (nx > HIPK_CHEB_MAXCOLS || !coef || !X || !G || !Out || Out == G) return -1;
   hipStream_t st = hip_stream ? (hipStream_t)hip_stream : A->ctx->stream;
   return csr_cheb_tiles(A, CSR_OP_CHEB_GATHER, st, nx, coef, X, ldx, G, ldg, Yk, ldk, Yprev, ldp, Out, ldo, nx == 1 ? 1 : (A->windowed ? 0 : -1));
}

/* max_i sum_j |a_ij| over the local rows: the infinity norm of the slab (of A' : the 1-norm of A) */
extern "C" int hipk_csr_abs_rowsum_max(hipk_csr *A, void *hip_stream, double *out) {
   if (!A || !out) return -1;
   if (A->kind != 0 || (A->dt != HIPK_F64 && A->dt != HIPK_F32)) return -44;
   hipStream_t st = hip_stream ? (hipStream_t)hip_stream : A->ctx->stream;
   return hipk_cheb_abs_rowsum_rows(A->ctx, st, A->dt, A->nrows, A->rowptr, A->values, out);
}

/* Gershgorin bounds of the local rows (include/primme_amd_kernels.h).  The Laplacian stencil form has diagonal 2 d and 2 d
 * off-diagonal entries -1 in its interior rows: [0, 4 d] whatever the slab (a slab without an interior row is one grid line
 * at most: the bound still encloses its discs). */
extern "C" int hipk_csr_gershgorin(hipk_csr *A, void *hip_stream, double out[2]) {
   if (!A || !out) return -1;
   if (A->kind == 1) {
      const int d = (A->sz > 1) ? 3 : (A->sy > 1 ? 2 : 1);
      if (A->nrows == 0) { out[0] = INFINITY; out[1] = -INFINITY; }
      else { out[0] = 0.0; out[1] = 4.0 * d; }
      return 0;
   }
   hipStream_t st = hip_stream ? (hipStream_t)hip_stream : A->ctx->stream;
   return hipk_cheb_gershgorin_rows(A->ctx, st, A->dt, A->nrows, A->row0, A->rowptr, A->colind, A->values, out);
}

/* y = A (a x), xout = a x, dot_dev[0] = xout' y with a = 1/sqrt(norm2_dev[0]) — see csr_stream_kernel<T, true>.
 * One column, CSR operators whose rows and input entries coincide (square, row-partitioned). */
extern "C" int hipk_csr_matvec_scaled(hipk_csr *A, hipk_ctx *ctx, const void *x, const double *norm2_dev,
      void *xout, void *y, double *dot_dev) {
   /* ctx: the CALLER's context (stream, reduction scratch, pinned mirror of the results) — the matrix may
    * have been created under another one */
   if (A->kind != 0 || A->x0 != A->row0 || A->xlen != A->nrows || x == xout || !ctx) return -1;
   if (HIPK_IS_Z(A->dt)) return -44;           /* the fused tail is real-arithmetic code (eigs_scalar.h) */
   hipStream_t st = ctx->stream;
   if ((A->halo_lo > 0 && !A->xlo) || (A->halo_hi > 0 && !A->xhi)) return -1;
   if (A->nrows == 0) {      /* an empty slab: the result is 0; no flagged launch, so the next wait drains the stream */
      ctx->tail_want = 0;
      if (ctx->tail_np2 > 0) { const int np = ctx->tail_np2; ctx->tail_np2 = 0; if (hipk_finalize_partials_t(ctx, ctx->tailp, np, 1, ctx->tail_norm2_out)) return -1; }
      HIPK_CHECK(hipMemsetAsync(dot_dev, 0, sizeof(double), st));
      double *mh = hipk_mirror_of(ctx, dot_dev);
      if (mh) { HIPK_CHECK(hipStreamSynchronize(st)); *mh = 0.0; }
      ctx->need_sync = 1;
      return 0;
   }
   const csr_route rt = csr_route_of(A, 1, CSR_OP_SCALED);
   const bool pat = rt.form == CSR_PAT;
   const int gx = pat ? hipk_pat_grid_kind(A->pat, ctx->num_cu, 1) : ((A->ntiles + 7) / 8) * 8;
   if (hipk_reserve_partials(ctx, (size_t)gx)) return -2;
   /* the tail of a block-size-1 iteration without second-stage launches (hipk_tail_defer): |t|^2 may still be np2 partial sums
    * (only the row-pattern kernel adds them itself; any other form gets them finished the separate way first), and the second
    * stage of t'At may be left to hipk_tail_finish */
   int np2 = 0;
   if (ctx->tail_np2 > 0) {
      if (pat && norm2_dev == ctx->tail_norm2_out) np2 = ctx->tail_np2;
      else {
         const int np = ctx->tail_np2;
         ctx->tail_np2 = 0;
         const int rc = hipk_finalize_partials_t(ctx, ctx->tailp, np, 1, ctx->tail_norm2_out);
         if (rc) return rc;
      }
   }
   const bool defer_dot = (ctx->tail_want & HIPK_TAIL_DOT) && ctx->tail_np3 == 0 && !hipk_inkernel_fin_mask();
   ctx->tail_want = 0;                                           /* one-shot */
   hipk_fin_args fa;
   if (defer_dot) memset(&fa, 0, sizeof(fa)); else fa = hipk_make_fin(ctx, dot_dev, HIPK_FIN_SPMV, gx, 1);
   const int pslot = hipk_prof_begin_s(HIPK_PROF_SPMV, st, rt.alg, rt.streamed);
   if (pat) {
      const int rc = hipk_pat_matvec(A->pat, st, gx, x, y, A->halo_lo, A->halo_hi, A->xlo, A->xhi, np2 > 0 ? ctx->tailp : norm2_dev, np2, xout, ctx->partials, &fa);
      hipk_prof_end(pslot, st);
      if (rc) return rc;
   } else {
      if (A->dt == HIPK_F64) csr_launch_scaled<double>(A, rt, st, gx, (const double *)x, norm2_dev, (double *)xout, (double *)y, ctx->partials, fa);
      else csr_launch_scaled<float>(A, rt, st, gx, (const float *)x, norm2_dev, (float *)xout, (float *)y, ctx->partials, fa);
      hipk_prof_end(pslot, st);
      HIPK_CHECK(hipGetLastError());
   }
   if (defer_dot) { ctx->tail_np3 = gx; ctx->tail_dot_out = dot_dev; return 0; }
   if (fa.enabled) return 0;
   return hipk_finalize_partials(ctx, ctx->partials, gx, 1, dot_dev);
}
