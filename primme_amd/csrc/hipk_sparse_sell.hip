/* hipk_sparse_sell.hip — the sliced-ELL form of a general CSR operator, SELL-64-256 (opt-in: HIPK_CSR_SLICED of
 * hipk_csr_create_opts, HIPK_SPMV_SELL=1 for hipk_csr_create; layout and converter: include/primme_amd_io.h, csr_tools.c).
 *
 * The row-tile kernels (hipk_sparse.hip) stage a tile's (value, column) pairs and row pointers in LDS and every lane then
 * walks its row through a chain of dependent LDS reads.  Here a lane owns one SLOT (a row of the length-sorted window) and
 * its entries lie column-major in the slice, so the wave's j-th load of values and of indices is one coalesced access that
 * goes from HBM straight to registers: no LDS, no barrier, no row pointer.  A workgroup is one window of 256 rows = 4 slices
 * = 4 waves; the windows are dealt to the XCDs in contiguous ranges (xcd_tile of hipk_sparse.hip) so that neighbouring
 * windows share their part of x in one L2.  x is gathered from global memory (narrow-band slices hit L2).
 *
 * Arithmetic: NC independent double accumulators per lane (the columns of a group); every column is ONE fma chain over the
 * row's entries in CSR order, so column c of a product does not depend on the width of the call and every run gives the
 * same bits.  The loop runs to the slice's width for the whole wave and loads unconditionally (padding is in range); an
 * entry past the lane's row length is skipped by a select on the length — never by multiplying with the stored 0, which
 * would let a NaN or Inf of x through.
 *
 * Measured on the LUNDA tiling of BASELINE configs[2] (profiles/sliced_spmm.json): SLOWER than the row tiles,
 * 0.90 of their speed at one column and 0.37 at eight (eight gathers per entry to eight columns of x, ldx apart).  Off by default.
 *
 * Memory: the form is kept BESIDE the CSR arrays (the Chebyshev step, the fused one-column product, the Gershgorin and
 * row-sum passes and the diagonal keep using those): padded * (s + 2 or 4) bytes + 3 bytes per slot + 12 per slice more. */
#include "hipk_internal.h"
#include "primme_amd_io.h"

#define SELL_MAX_PADDING 1.25

struct hipk_sell {
   hipk_ctx *ctx;
   hipk_dtype dt;
   int idx16;
   int64_t m, nnz, nslices, padded, total;
   int nwin;
   int64_t *base;       /* device */
   int32_t *cmin;
   uint8_t *perm;
   uint16_t *len;
   void *val, *idx;
};

extern "C" void hipk_sell_destroy(hipk_sell *B);

struct SellShift { double s[64]; int on; };

__device__ __forceinline__ int sell_xcd_window(int b, int nwin) {
   const int per = (nwin + 7) >> 3;
   return (b & 7) * per + (b >> 3);
}

template <typename T, typename IT, int NC>
__global__ void __launch_bounds__(HIPK_BLOCK)
sell_kernel(const int64_t *__restrict__ base, const int32_t *__restrict__ cmin, const uint8_t *__restrict__ perm,
      const uint16_t *__restrict__ len, const T *__restrict__ val, const IT *__restrict__ idx, int nwin, int64_t nslices,
      int64_t m, int64_t row0, const T *__restrict__ x, int64_t ldx, T *__restrict__ y, int64_t ldy, int ncols, SellShift sh) {
   const int win = sell_xcd_window(blockIdx.x, nwin);
   if (win >= nwin) return;
   const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
   const int64_t s = (int64_t)win * 4 + wave;
   if (s >= nslices) return;                             /* the ragged last window (no barrier in this kernel) */
   const int64_t b0 = base[s];
   const int width = (int)((base[s + 1] - b0) >> 6);
   const int64_t p = s * 64 + lane;                      /* < 64 nslices: perm and len are that long */
   const int mylen = len[p];
   const int64_t row = (int64_t)win * 256 + perm[p];
   const int64_t xoff = (int64_t)cmin[s] - row0;         /* x entry of stored index i: xoff + i */
   const T *__restrict__ vp = val + b0 + lane;
   const IT *__restrict__ ip = idx + b0 + lane;
   for (int c0 = 0; c0 < ncols; c0 += NC) {
      /* columns past ncols alias the last valid one (computed, never stored): no branch in the gather loop */
      const T *xc[NC];
#pragma unroll
      for (int c = 0; c < NC; c++) xc[c] = x + (size_t)((c0 + c < ncols) ? c0 + c : ncols - 1) * ldx + xoff;
      double acc[NC];
#pragma unroll
      for (int c = 0; c < NC; c++) acc[c] = 0.0;
      int j = 0;
      for (; j + 4 <= width; j += 4) {                   /* 4 entries per trip: 4 NC independent gathers in flight */
         T v[4];
         uint32_t ix[4];
#pragma unroll
         for (int u = 0; u < 4; u++) { v[u] = vp[(j + u) * 64]; ix[u] = (uint32_t)ip[(j + u) * 64]; }
#pragma unroll
         for (int u = 0; u < 4; u++)
#pragma unroll
            for (int c = 0; c < NC; c++) {
               const double t = fma((double)v[u], (double)xc[c][ix[u]], acc[c]);
               acc[c] = (j + u < mylen) ? t : acc[c];
            }
      }
      for (; j < width; j++) {
         const double v = (double)vp[j * 64];
         const uint32_t ix = (uint32_t)ip[j * 64];
#pragma unroll
         for (int c = 0; c < NC; c++) {
            const double t = fma(v, (double)xc[c][ix], acc[c]);
            acc[c] = (j < mylen) ? t : acc[c];
         }
      }
      if (p < m) {
#pragma unroll
         for (int c = 0; c < NC; c++)
            if (c0 + c < ncols) {
               double out = acc[c];
               if (sh.on) out = fma(-sh.s[c0 + c], (double)x[row + (size_t)(c0 + c) * ldx], out);
               y[row + (size_t)(c0 + c) * ldy] = (T)out;
            }
      }
   }
}

/* builds the form when the matrix qualifies by its padding; *out stays NULL (return 0) when it does not */
extern "C" int hipk_sell_build(hipk_ctx *ctx, hipk_dtype dt, int64_t m, const int32_t *rp, const int32_t *ci, const void *val, hipk_sell **out) {
   *out = NULL;
   if (dt != HIPK_F64 && dt != HIPK_F32) return 0;
   const size_t es = hipk_elem_size(dt);
   primme_amd_sliced *S = NULL;
   const int rc = primme_amd_csr_to_sliced(m, rp, ci, val, es, SELL_MAX_PADDING, &S);
   if (rc == 1 || rc == -4) return 0;                    /* too much padding / a row too long for the form: the row tiles serve it */
   if (rc) return -2;
   if ((S->m + 255) / 256 >= (int64_t)INT32_MAX / 8) { primme_amd_sliced_free(S); return 0; }
   hipk_sell *B = (hipk_sell *)calloc(1, sizeof(hipk_sell));
   if (!B) { primme_amd_sliced_free(S); return -2; }
   B->ctx = ctx; B->dt = dt; B->idx16 = S->idx16; B->m = S->m; B->nnz = S->nnz; B->nslices = S->nslices; B->padded = S->padded;
   B->total = S->base[S->nslices];
   B->nwin = (int)((S->m + 255) / 256);
   const size_t is = S->idx16 ? 2 : 4, tot = (size_t)(B->total > 0 ? B->total : 1), nslots = (size_t)S->nslices * 64;
   int bad = hipk_malloc(ctx, (size_t)(S->nslices + 1) * 8, (void **)&B->base) || hipk_malloc(ctx, (size_t)S->nslices * 4, (void **)&B->cmin) ||
             hipk_malloc(ctx, nslots, (void **)&B->perm) || hipk_malloc(ctx, nslots * 2, (void **)&B->len) ||
             hipk_malloc(ctx, tot * es, &B->val) || hipk_malloc(ctx, tot * is, &B->idx);
   int rcu = 0;
   if (!bad)
      rcu = hipk_upload(ctx, B->base, S->base, (size_t)(S->nslices + 1) * 8) || hipk_upload(ctx, B->cmin, S->cmin, (size_t)S->nslices * 4) ||
            hipk_upload(ctx, B->perm, S->perm, nslots) || hipk_upload(ctx, B->len, S->len, nslots * 2) ||
            hipk_upload(ctx, B->val, S->val, tot * es) || hipk_upload(ctx, B->idx, S->idx, tot * is);
   primme_amd_sliced_free(S);
   if (bad || rcu) { hipk_sell_destroy(B); return bad ? -2 : -1; }
   *out = B;
   return 0;
}

extern "C" void hipk_sell_destroy(hipk_sell *B) {
   if (!B) return;
   if (B->base) (void)hipFree(B->base);
   if (B->cmin) (void)hipFree(B->cmin);
   if (B->perm) (void)hipFree(B->perm);
   if (B->len) (void)hipFree(B->len);
   if (B->val) (void)hipFree(B->val);
   if (B->idx) (void)hipFree(B->idx);
   free(B);
}

extern "C" double hipk_sell_padding(const hipk_sell *B) { return B && B->nnz > 0 ? (double)B->padded / (double)B->nnz : 0.0; }
extern "C" int hipk_sell_index_bytes(const hipk_sell *B) { return B->idx16 ? 2 : 4; }

/* bytes one product of ncols columns moves through HBM: the padded (value, index) entries once (the later column groups of a
 * wide call re-read them from L2), slot and slice records, x and y */
extern "C" double hipk_sell_bytes(const hipk_sell *B, int ncols) {
   const double es = B->dt == HIPK_F64 ? 8 : 4;
   return (double)B->padded * (es + (B->idx16 ? 2 : 4)) + (double)B->nslices * (64 * 3 + 12) + 2.0 * (double)B->m * es * ncols;
}

template <typename T, typename IT>
static void sell_launch(const hipk_sell *B, hipStream_t st, int64_t row0, const T *x, int64_t ldx, T *y, int64_t ldy, int ncols, const SellShift &sh) {
   const int gx = ((B->nwin + 7) / 8) * 8;
#define SELL_GO(NCV) hipLaunchKernelGGL((sell_kernel<T, IT, NCV>), dim3(gx), dim3(HIPK_BLOCK), 0, st, B->base, B->cmin, B->perm, B->len, \
      (const T *)B->val, (const IT *)B->idx, B->nwin, B->nslices, B->m, row0, x, ldx, y, ldy, ncols, sh)
   if (ncols == 1) SELL_GO(1);
   else if (ncols == 2) SELL_GO(2);
   else if (ncols <= 4) SELL_GO(4);
   else SELL_GO(8);
#undef SELL_GO
}

/* y = A x, or A x - shift[c] x(:,c) when shift_host != NULL (then ncols <= 64); x and y are the row slab (no halo) */
extern "C" int hipk_sell_matvec(const hipk_sell *B, void *hip_stream, int64_t row0, const void *x, int64_t ldx, void *y, int64_t ldy, int ncols,
      const double *shift_host) {
   if (ncols <= 0 || B->m == 0) return 0;
   if (shift_host && ncols > 64) return -1;
   hipStream_t st = (hipStream_t)hip_stream;
   SellShift sh;
   sh.on = shift_host != NULL;
   for (int c = 0; c < 64; c++) sh.s[c] = (shift_host && c < ncols) ? shift_host[c] : 0.0;
   if (B->dt == HIPK_F64) {
      if (B->idx16) sell_launch<double, uint16_t>(B, st, row0, (const double *)x, ldx, (double *)y, ldy, ncols, sh);
      else sell_launch<double, int32_t>(B, st, row0, (const double *)x, ldx, (double *)y, ldy, ncols, sh);
   } else {
      if (B->idx16) sell_launch<float, uint16_t>(B, st, row0, (const float *)x, ldx, (float *)y, ldy, ncols, sh);
      else sell_launch<float, int32_t>(B, st, row0, (const float *)x, ldx, (float *)y, ldy, ncols, sh);
   }
   HIPK_CHECK(hipGetLastError());
   return 0;
}
