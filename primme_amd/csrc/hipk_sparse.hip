/* hipk_sparse.hip — the user matvec on the device: CSR SpMV/SpMM (LDS-staged
 * row tiles, "CSR-stream"), a wave-per-row path for long rows, a matrix-free
 * Laplacian stencil; kernels and their launchers.  The hipk_csr object that routes the products
 * here is in hipk_csr.hip, what the two units share in hipk_sparse_dev.h.
 *
 * Replaces the hipsparseSpMM callback of reference examples/ex_eigs_dhipblas.c:239-264
 * (which re-queries buffer sizes and rebuilds dense descriptors on every call) and
 * the SPARSKIT amux loop of tests/COMMON/mat.c:64-90.
 *
 * CSR-stream: the host bins consecutive rows into tiles holding <= TILE_NNZ
 * nonzeros and <= 256 rows.  A workgroup streams its tile's (value, column)
 * pairs with fully coalesced loads, multiplies by the gathered x entries, parks
 * the products in LDS, and then one lane per row adds that row's LDS segment.
 * HBM traffic is the algorithmic minimum nnz*(s+4) + rows*(4 + 2s); the x gather
 * is served by L2 (tiles are assigned to XCDs in contiguous row ranges so that
 * neighbouring tiles share their x window in one L2).
 */
#include "hipk_sparse_dev.h"

/* CSR-stream, one column at a time.  The chain of dependent memory round trips per tile is what
 * bounds this kernel, not the bytes: {r0,r1,p0,p1} come in one 16-byte load, a lane then issues
 * ALL of its (value, column) loads of the tile before the first gather (indices clamped instead
 * of predicated, so nothing branches around a load), all gathers before the first product, and
 * the row pointers of the summing phase are fetched before the barrier.
 * FUSED (one column): the input is the un-normalised new basis vector t and |t|^2 sits in HBM
 * (norm2[0]); a = 1/sqrt(|t|^2) is applied to every gathered entry on the fly, the normalised
 * vector is written to xout for the rows this tile owns (xout != x: other tiles still gather from
 * x), and the tile's part of xout' y goes to partials[blockIdx.x].  Replaces the separate
 * normalisation pass and the two-vector inner product t'At of the one-synchronisation GD
 * iteration (eigs_conv.c); same arithmetic per element as scale_rsqrt_kernel + this kernel. */
/* NTM: the (value, index) stream with the non-temporal hint — for matrices too large to stay in the 256 MiB Infinity
 * Cache between two products (the launcher decides by the size of the stream); smaller ones are left to be cached. */
template <typename T, bool FUSED, bool C16, bool NTM>
__global__ void __launch_bounds__(HIPK_BLOCK)
csr_stream_kernel(const int4 *__restrict__ tileinfo, int ntiles, const int32_t *__restrict__ rowptr,
      const int32_t *__restrict__ colind, const uint16_t *__restrict__ col16, int64_t c16off,
      const T *__restrict__ val, const T *__restrict__ x,
      int64_t ldx, T *__restrict__ y, int64_t ldy, int ncols, int64_t row0, int64_t nrows,
      int64_t halo_lo, int64_t halo_hi, const T *__restrict__ xlo, const T *__restrict__ xhi,
      int64_t ld_lo, int64_t ld_hi, const double *__restrict__ norm2, T *__restrict__ xout,
      double *__restrict__ partials, hipk_fin_args fa) {
   __shared__ double prod[TILE_NNZ];
   __shared__ int s_last;
   const int tile = xcd_tile(blockIdx.x, ntiles);
   double dotp = 0.0;
   if (tile < ntiles) {
      const int4 ti = tileinfo[tile];
      const int r0 = ti.x, r1 = ti.y, p0 = ti.z, nz = ti.w - ti.z;
      const bool local = (halo_lo == 0 && halo_hi == 0);
      const double a = (FUSED && norm2) ? 1.0 / sqrt(norm2[0]) : 1.0;   /* norm2 == NULL: no scaling (xout = x) */
      if (nz <= TILE_NNZ) {
         /* row segment of this lane's row: fetched now, used after the barrier */
         const int r = r0 + threadIdx.x;
         const int rc = r < r1 ? r : r1 - 1;
         const int sa = rowptr[rc] - p0, sb = rowptr[rc + 1] - p0;
         /* the tile's (value, column) pairs: all loads in flight at once */
         double v[TILE_PER_LANE];
         int32_t cidx[TILE_PER_LANE];
#pragma unroll
         for (int u = 0; u < TILE_PER_LANE; u++) {
            const int q = threadIdx.x + u * HIPK_BLOCK;
            const int qc = q < nz ? q : (nz > 0 ? nz - 1 : 0);   /* an all-empty tile reads the padded element */
            v[u] = (double)(NTM ? __builtin_nontemporal_load(val + p0 + qc) : val[p0 + qc]);
            /* C16 (a template parameter: exactly one index stream is loaded): global column = row0 + r0 - c16back + entry;
             * an empty tile reads a neighbour's entry against its own base, so its (unused) gather goes to a valid row */
            if (C16) cidx[u] = (int32_t)(NTM ? __builtin_nontemporal_load(col16 + p0 + qc) : col16[p0 + qc]);   /* raw: any arithmetic here would make the batch wait load by load */
            else cidx[u] = NTM ? __builtin_nontemporal_load(colind + p0 + qc) : colind[p0 + qc];
         }
         if (C16) {
            const int32_t cbase = (int32_t)(c16off + r0);
#pragma unroll
            for (int u = 0; u < TILE_PER_LANE; u++) cidx[u] = nz > 0 ? cbase + cidx[u] : (int32_t)row0;
         }
         for (int c = 0; c < ncols; c++) {
            const T *xc = x + (size_t)c * ldx;
            const T *xloc = xlo ? xlo + (size_t)c * ld_lo : xc;
            const T *xhic = xhi ? xhi + (size_t)c * ld_hi : xc;
            double xg[TILE_PER_LANE];
            if (local) {
#pragma unroll
               for (int u = 0; u < TILE_PER_LANE; u++) xg[u] = (double)xc[(int64_t)cidx[u] - row0];
            } else {
#pragma unroll
               for (int u = 0; u < TILE_PER_LANE; u++) xg[u] = fetch_x<T>(xc, xloc, xhic, row0, nrows, halo_lo, (int64_t)cidx[u]);
            }
            double xown = 0.0;
            if (FUSED && r < r1) xown = (double)(T)(a * (double)xc[r]);    /* rows are local entries: r indexes the slab */
#pragma unroll
            for (int u = 0; u < TILE_PER_LANE; u++) {
               const int q = threadIdx.x + u * HIPK_BLOCK;
               const double xv = FUSED ? (double)(T)(a * xg[u]) : xg[u];
               if (q < nz) prod[q] = v[u] * xv;
            }
            __syncthreads();
            if (r < r1) {
               double s = 0.0;
               for (int q = sa; q < sb; q++) s += prod[q];
               const T yt = (T)s;
               y[r + (size_t)c * ldy] = yt;
               if (FUSED) { xout[r] = (T)xown; dotp = fma(xown, (double)yt, dotp); }
            }
            if (c + 1 < ncols) __syncthreads();
         }
      } else {
         /* a tile that is one long row: the whole workgroup reduces it */
         for (int c = 0; c < ncols; c++) {
            const T *xc = x + (size_t)c * ldx;
            const T *xloc = xlo ? xlo + (size_t)c * ld_lo : xc;
            const T *xhic = xhi ? xhi + (size_t)c * ld_hi : xc;
            for (int r = r0; r < r1; r++) {
               const int qa = rowptr[r], qb = rowptr[r + 1];
               double s = 0.0;
               for (int q = qa + threadIdx.x; q < qb; q += HIPK_BLOCK) {
                  const double xg = fetch_x<T>(xc, xloc, xhic, row0, nrows, halo_lo, (int64_t)colind[q]);
                  s = fma((double)val[q], FUSED ? (double)(T)(a * xg) : xg, s);
               }
               s = hipk_wave_sum(s);
               if ((threadIdx.x & 63) == 0) prod[threadIdx.x >> 6] = s;
               __syncthreads();
               if (threadIdx.x == 0) {
                  const T yt = (T)((prod[0] + prod[1]) + (prod[2] + prod[3]));
                  y[r + (size_t)c * ldy] = yt;
                  if (FUSED) { const T xo = (T)(a * (double)xc[r]); xout[r] = xo; dotp = fma((double)xo, (double)yt, dotp); }
               }
               __syncthreads();
            }
         }
      }
   }
   if (FUSED) {
      __shared__ double red[HIPK_BLOCK / HIPK_WAVE];
      __syncthreads();
      const double t = hipk_wave_sum(dotp);
      if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
      __syncthreads();
      if (threadIdx.x == 0) hipk_pstore(fa, partials + blockIdx.x, (red[0] + red[1]) + (red[2] + red[3]));
      hipk_inkernel_finalize(partials, 1, gridDim.x, fa, &s_last);
   }
}

/* Block of vectors (the JDQMR / block Davidson SpMM).  The tile's (value, column) pairs are
 * staged ONCE in LDS with coalesced loads (one barrier per tile, not two per column); then one
 * lane per (row, group of NC columns) walks its row in LDS and gathers x for its NC columns with
 * independent accumulators, so a lane keeps ~NC x row-length gathers in flight and nothing is
 * re-read from HBM for the second and later columns. */
template <typename T, int NC>
__global__ void __launch_bounds__(HIPK_BLOCK)
csr_rows_block_kernel(const int32_t *__restrict__ tiles, int ntiles, const int32_t *__restrict__ rowptr,
      const int32_t *__restrict__ colind, const T *__restrict__ val, const T *__restrict__ x,
      int64_t ldx, T *__restrict__ y, int64_t ldy, int ncols, int64_t row0, int64_t nrows,
      int64_t halo_lo, int64_t halo_hi, const T *__restrict__ xlo, const T *__restrict__ xhi,
      int64_t ld_lo, int64_t ld_hi) {
   __shared__ T sval[TILE_NNZ];
   __shared__ int32_t scol[TILE_NNZ];
   __shared__ int rp[TILE_ROWS + 1];
   const int tile = xcd_tile(blockIdx.x, ntiles);
   if (tile >= ntiles) return;
   const int r0 = tiles[tile], r1 = tiles[tile + 1];
   const int p0 = rowptr[r0], p1 = rowptr[r1];
   const int nz = p1 - p0, nr = r1 - r0;
   const bool local = (halo_lo == 0 && halo_hi == 0);

   if (nz <= TILE_NNZ) {
      {  /* all of this lane's (value, column) loads in flight at once: indices clamped, not predicated */
         T tv[TILE_PER_LANE];
         int32_t tc[TILE_PER_LANE];
         csr_tile_loads<T, false>(val, colind, NULL, p0, nz, tv, tc);
         const int rr = threadIdx.x <= nr ? threadIdx.x : nr;
         const int rpv = rowptr[r0 + rr] - p0;
#pragma unroll
         for (int u = 0; u < TILE_PER_LANE; u++) {
            const int q = threadIdx.x + u * HIPK_BLOCK;
            if (q < nz) { sval[q] = tv[u]; scol[q] = tc[u]; }
         }
         if (threadIdx.x <= nr) rp[threadIdx.x] = rpv;
         if (threadIdx.x == 0 && nr == TILE_ROWS) rp[TILE_ROWS] = rowptr[r0 + TILE_ROWS] - p0;
      }
      __syncthreads();
      const int ngroups = (ncols + NC - 1) / NC;
      for (int idx = threadIdx.x; idx < nr * ngroups; idx += HIPK_BLOCK) {
         const int g = idx / nr, r = idx - g * nr, c0 = g * NC;
         double acc[NC];
#pragma unroll
         for (int c = 0; c < NC; c++) acc[c] = 0.0;
         const int qa = rp[r], qb = rp[r + 1];
         if (local) {
            /* columns past ncols alias the last valid one (computed, never stored): no branches
             * in the gather loop; 4 row entries per trip = 4*NC independent gathers in flight */
            const T *xg[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) xg[c] = x + (size_t)((c0 + c < ncols) ? c0 + c : ncols - 1) * ldx - row0;
            const int64_t self = row0;   /* any owned entry: multiplied by zero */
            for (int q = qa; q < qb; q += 4) {
               double v[4];
               int64_t gc[4];
#pragma unroll
               for (int u = 0; u < 4; u++) {
                  const bool ok = q + u < qb;
                  v[u] = ok ? (double)sval[ok ? q + u : qa] : 0.0;
                  gc[u] = ok ? (int64_t)scol[ok ? q + u : qa] : self;
               }
#pragma unroll
               for (int u = 0; u < 4; u++)
#pragma unroll
                  for (int c = 0; c < NC; c++) acc[c] = fma(v[u], (double)xg[c][gc[u]], acc[c]);
            }
         } else {
            for (int q = qa; q < qb; q++) {
               const double v = (double)sval[q];
               const int64_t gcol = scol[q];
#pragma unroll
               for (int c = 0; c < NC; c++)
                  if (c0 + c < ncols)
                     acc[c] = fma(v, fetch_x<T>(x + (size_t)(c0 + c) * ldx, xlo ? xlo + (size_t)(c0 + c) * ld_lo : x,
                                                 xhi ? xhi + (size_t)(c0 + c) * ld_hi : x, row0, nrows, halo_lo, gcol), acc[c]);
            }
         }
#pragma unroll
         for (int c = 0; c < NC; c++)
            if (c0 + c < ncols) y[r0 + r + (size_t)(c0 + c) * ldy] = (T)acc[c];
      }
   } else {
      __shared__ double red[HIPK_BLOCK / HIPK_WAVE];
      for (int c = 0; c < ncols; c++) {
         const T *xc = x + (size_t)c * ldx;
         const T *xloc = xlo ? xlo + (size_t)c * ld_lo : xc;
         const T *xhic = xhi ? xhi + (size_t)c * ld_hi : xc;
         for (int r = r0; r < r1; r++) {
            const int a = rowptr[r], b = rowptr[r + 1];
            double sum = 0.0;
            for (int q = a + threadIdx.x; q < b; q += HIPK_BLOCK)
               sum = fma((double)val[q], fetch_x<T>(xc, xloc, xhic, row0, nrows, halo_lo, (int64_t)colind[q]), sum);
            sum = hipk_wave_sum(sum);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
            __syncthreads();
            if (threadIdx.x == 0) y[r + (size_t)c * ldy] = (T)((red[0] + red[1]) + (red[2] + red[3]));
            __syncthreads();
         }
      }
   }
}

/* The same with the x WINDOW of the tile staged in LDS.  For banded, block-diagonal and 2-D
 * stencil matrices the column indices of a tile's nonzeros span a few hundred rows of x: that slice
 * of the block of vectors ([cmin, cmin + cw) x ncols, at most XS_MAX values) is fetched from HBM
 * with coalesced loads — every x entry the tile needs comes in ONCE per tile instead of once per
 * nonzero through a scattered 8-byte L2 access — and the row walk gathers from LDS.  Tiles whose
 * window is too wide or reaches outside the owned slab (twin.y == 0) use the global gathers.
 * shift != NULL: y = A x - shift[c] x(:,c), the first update of the projected operator in the
 * JDQMR inner iteration (reference inner_solve.c:853-858) fused into the operator. */
struct SpmmShift { double s[64]; int on; int nosplit; int evenstride; };
struct SpmmNoEp {};
template <typename T, bool CHEB> struct SpmmEp { typedef SpmmNoEp type; };
template <typename T> struct SpmmEp<T, true> { typedef SpmmCheb<T> type; };
template <typename T, bool CHEB>
__device__ __forceinline__ double spmm_epilogue(const typename SpmmEp<T, CHEB>::type &ep, double sum, int64_t row, int c) {
   if constexpr (CHEB) {
      double o = ep.cf.cx[c] * (double)ep.xr[row + (size_t)c * ep.ldr];
      if (ep.yk) o = fma(ep.cf.cy[c], (double)ep.yk[row + (size_t)c * ep.ldk], o);
      if (ep.yp) o = fma(ep.cf.cp[c], (double)ep.yp[row + (size_t)c * ep.ldp], o);
      return fma(ep.cf.cw[c], sum, o);
   } else {
      return sum;
   }
}
template <typename T, bool CHEB>
__device__ __forceinline__ bool spmm_seq(const typename SpmmEp<T, CHEB>::type &ep) {
   if constexpr (CHEB) return ep.seq > 0; else return false;
}
/* acc + round(v x): two roundings, never contracted into one fma */
__device__ __forceinline__ double spmm_add_rounded_product(double acc, double v, double x) {
#pragma clang fp contract(off)
   const double p = v * x;
   return acc + p;
}
template <typename T, int NC, int XS, bool C16, bool CHEB = false>
__global__ void __launch_bounds__(HIPK_BLOCK)
csr_window_block_kernel(const int4 *__restrict__ tileinfo, const int2 *__restrict__ twin, int ntiles,
      const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colind, const uint16_t *__restrict__ col16, int64_t c16off,
      const T *__restrict__ val,
      const T *__restrict__ x, int64_t ldx, T *__restrict__ y, int64_t ldy, int ncols, int64_t row0,
      SpmmShift sh, typename SpmmEp<T, CHEB>::type ep) {
   __shared__ T sval[TILE_NNZ];
   __shared__ int32_t scol[TILE_NNZ];
   __shared__ int rp[TILE_ROWS + 1];
   __shared__ double xs[XS];                 /* xs[w * ncols + c] = x(cmin + w, c) */
   const int tile = xcd_tile(blockIdx.x, ntiles);
   if (tile >= ntiles) return;
   const int4 ti = tileinfo[tile];
   const int2 tw = twin[tile];
   const int r0 = ti.x, r1 = ti.y, p0 = ti.z, nz = ti.w - ti.z, nr = r1 - r0;
   const int cmin = tw.x, cw = tw.y;
   /* LDS rows of the window are `xst` doubles apart, xst ODD: the lanes of a wave walk different rows of the matrix and read
    * the window at unrelated row numbers — with a stride of ncols = 8 doubles (64 bytes = 16 banks) only four bank groups
    * exist and a 32-lane read serialises up to eight-fold; with 9 the 32 lanes hit 32 distinct bank pairs (round 6:
    * profiles/r06_spmm_window_stride.txt) */
   const int xst = sh.evenstride ? ncols : (ncols | 1);
   const bool win = cw > 0 && cw * xst <= XS && nz <= TILE_NNZ;
   if (nz <= TILE_NNZ) {
      {  /* every load of the tile — (value, column) pairs, row pointers, the x window — is issued before
          * the first LDS store: indices clamped, not predicated, so nothing branches around a load */
         T tv[TILE_PER_LANE];
         int32_t tc[TILE_PER_LANE];
         T xw[(XS + HIPK_BLOCK - 1) / HIPK_BLOCK];
         csr_tile_loads<T, C16>(val, colind, col16, p0, nz, tv, tc);      /* C16 raw: the base is added when the entry goes to LDS */
         const int rr = threadIdx.x <= nr ? threadIdx.x : nr;
         const int rpv = rowptr[r0 + rr] - p0;
         const int nxw = win ? cw * ncols : 0;
         if (win) {
#pragma unroll
            for (int u = 0; u < (XS + HIPK_BLOCK - 1) / HIPK_BLOCK; u++) {
               const int idx = threadIdx.x + u * HIPK_BLOCK;
               const int ic = idx < nxw ? idx : nxw - 1;
               const int c = ic / cw, w = ic - c * cw;          /* coalesced along the window for each column */
               xw[u] = x[(int64_t)cmin - row0 + w + (size_t)c * ldx];
            }
         }
         const int32_t cadj = (C16 ? (int32_t)(c16off + r0) : 0) - (win ? cmin : 0);   /* stored column: global, or window-relative */
#pragma unroll
         for (int u = 0; u < TILE_PER_LANE; u++) {
            const int q = threadIdx.x + u * HIPK_BLOCK;
            if (q < nz) { sval[q] = tv[u]; scol[q] = tc[u] + cadj; }
         }
         if (threadIdx.x <= nr) rp[threadIdx.x] = rpv;
         if (threadIdx.x == 0 && nr == TILE_ROWS) rp[TILE_ROWS] = rowptr[r0 + TILE_ROWS] - p0;
         if (win) {
#pragma unroll
            for (int u = 0; u < (XS + HIPK_BLOCK - 1) / HIPK_BLOCK; u++) {
               const int idx = threadIdx.x + u * HIPK_BLOCK;
               if (idx < nxw) { const int c = idx / cw, w = idx - c * cw; xs[w * xst + c] = (double)xw[u]; }   /* LDS rows are xst apart */
            }
         }
      }
      __syncthreads();
      const int ngroups = (ncols + NC - 1) / NC;
      /* A tile of 2048 nonzeros has ~120 rows of 17: with one lane per (row, column group) half of the workgroup idles
       * through the row walk, a chain of dependent LDS reads.  When the work fits twice, two adjacent lanes share a row:
       * each walks half of its nonzeros and the halves meet in a shuffle (fixed order: low half + high half). */
      const bool seq = spmm_seq<T, CHEB>(ep);
      const int split = (2 * nr * ngroups <= HIPK_BLOCK && !sh.nosplit && !seq) ? 2 : 1;
      for (int idx0 = threadIdx.x; idx0 < nr * ngroups * split; idx0 += HIPK_BLOCK) {
         const int idx = idx0 / split, half = idx0 - idx * split;
         const int g = idx / nr, r = idx - g * nr, c0 = g * NC;
         double acc[NC];
#pragma unroll
         for (int c = 0; c < NC; c++) acc[c] = 0.0;
         int qa = rp[r], qb = rp[r + 1];
         if (split == 2) { const int qm = qa + (qb - qa + 1) / 2; if (half) qa = qm; else qb = qm; }
         if (seq) {
            /* one column (c0 = 0, the lane's other accumulators stay 0): csr_stream_kernel's order and roundings */
            const T *xg = x - row0;
            if (win) for (int q = qa; q < qb; q++) acc[0] = spmm_add_rounded_product(acc[0], (double)sval[q], xs[scol[q] * xst]);
            else for (int q = qa; q < qb; q++) acc[0] = spmm_add_rounded_product(acc[0], (double)sval[q], (double)xg[(int64_t)scol[q]]);
         } else if (win) {
            int cofs[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) cofs[c] = (c0 + c < ncols) ? c0 + c : ncols - 1;
            for (int q = qa; q < qb; q++) {
               const double v = (double)sval[q];
               const double *xr = xs + scol[q] * xst;
#pragma unroll
               for (int c = 0; c < NC; c++) acc[c] = fma(v, xr[cofs[c]], acc[c]);
            }
         } else {
            const T *xg[NC];
#pragma unroll
            for (int c = 0; c < NC; c++) xg[c] = x + (size_t)((c0 + c < ncols) ? c0 + c : ncols - 1) * ldx - row0;
            const int64_t self = row0;   /* any owned entry: multiplied by zero */
            for (int q = qa; q < qb; q += 4) {
               double v[4];
               int64_t gc[4];
#pragma unroll
               for (int u = 0; u < 4; u++) {
                  const bool ok = q + u < qb;
                  v[u] = ok ? (double)sval[ok ? q + u : qa] : 0.0;
                  gc[u] = ok ? (int64_t)scol[ok ? q + u : qa] : self;
               }
#pragma unroll
               for (int u = 0; u < 4; u++)
#pragma unroll
                  for (int c = 0; c < NC; c++) acc[c] = fma(v[u], (double)xg[c][gc[u]], acc[c]);
            }
         }
         if (split == 2) {
            /* (2 nr ngroups <= 256: one trip, both lanes of a pair are in it) */
#pragma unroll
            for (int c = 0; c < NC; c++) { const double o = __shfl_xor(acc[c], 1); acc[c] = half ? o + acc[c] : acc[c] + o; }
            if (half) continue;
         }
#pragma unroll
         for (int c = 0; c < NC; c++)
            if (c0 + c < ncols) {
               double out = acc[c];
               if (sh.on) out = fma(-sh.s[c0 + c], (double)x[(int64_t)(r0 + r) + (size_t)(c0 + c) * ldx], out);
               out = spmm_epilogue<T, CHEB>(ep, out, (int64_t)(r0 + r), c0 + c);
               y[r0 + r + (size_t)(c0 + c) * ldy] = (T)out;
            }
      }
   } else {
      __shared__ double red[HIPK_BLOCK / HIPK_WAVE];
      for (int c = 0; c < ncols; c++) {
         const T *xc = x + (size_t)c * ldx - row0;
         for (int r = r0; r < r1; r++) {
            const int a = rowptr[r], b = rowptr[r + 1];
            double sum = 0.0;
            for (int q = a + threadIdx.x; q < b; q += HIPK_BLOCK) sum = fma((double)val[q], (double)xc[colind[q]], sum);
            sum = hipk_wave_sum(sum);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
            __syncthreads();
            if (threadIdx.x == 0) {
               double out = (red[0] + red[1]) + (red[2] + red[3]);
               if (sh.on) out = fma(-sh.s[c], (double)xc[row0 + r], out);
               out = spmm_epilogue<T, CHEB>(ep, out, (int64_t)r, c);
               y[r + (size_t)c * ldy] = (T)out;
            }
            __syncthreads();
         }
      }
   }
}

/* Laplacian stencil: diag 2*dims, -1 to each grid neighbour, Dirichlet boundary. */
template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
stencil_kernel(int sx, int sy, int sz, int64_t row0, int64_t nrows, const T *__restrict__ x,
      int64_t ldx, T *__restrict__ y, int64_t ldy, int ncols, int64_t halo_lo, int64_t halo_hi,
      const T *__restrict__ xlo, const T *__restrict__ xhi, int64_t ld_lo, int64_t ld_hi) {
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   const int64_t plane = (int64_t)sx * sy;
   const double dg = (sz > 1) ? 6.0 : (sy > 1 ? 4.0 : 2.0);
   for (int c = 0; c < ncols; c++) {
      const T *xc = x + (size_t)c * ldx;
      const T *xloc = xlo ? xlo + (size_t)c * ld_lo : xc;
      const T *xhic = xhi ? xhi + (size_t)c * ld_hi : xc;
      T *yc = y + (size_t)c * ldy;
      for (int64_t l = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; l < nrows; l += stride) {
         const int64_t g = row0 + l;
         const int ix = (int)(g % sx);
         const int iy = (int)((g / sx) % sy);
         const int iz = (int)(g / plane);
         double s = dg * (double)xc[l];
#define NB(gn) fetch_x<T>(xc, xloc, xhic, row0, nrows, halo_lo, (gn))
         if (ix > 0) s -= NB(g - 1);
         if (ix < sx - 1) s -= NB(g + 1);
         if (sy > 1) {
            if (iy > 0) s -= NB(g - sx);
            if (iy < sy - 1) s -= NB(g + sx);
         }
         if (sz > 1) {
            if (iz > 0) s -= NB(g - plane);
            if (iz < sz - 1) s -= NB(g + plane);
         }
#undef NB
         yc[l] = (T)s;
      }
   }
}

/* ---- launchers: what csr_route (hipk_csr.hip) chose, launched; the caller checks hipGetLastError ---- */
template <typename T>
void csr_launch_stencil(const hipk_csr *A, hipStream_t st, const T *x, int64_t ldx, T *y, int64_t ldy, int ncols) {
   const int gx = hipk_grid_for_rows(A->ctx, A->nrows, HIPK_BLOCK, 8);
   hipLaunchKernelGGL(stencil_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, st, A->sx, A->sy, A->sz, A->row0, A->nrows, x, ldx, y, ldy, ncols,
         A->halo_lo, A->halo_hi, (const T *)A->xlo, (const T *)A->xhi, A->ld_lo, A->ld_hi);
}

template <typename T, bool FUSED>
static void launch_stream(const hipk_csr *A, const csr_route &rt, hipStream_t st, int gx, const T *x, int64_t ldx, T *y, int64_t ldy,
      const double *norm2, T *xout, double *partials, const hipk_fin_args &fa) {
#define LAUNCH_STREAM(C16V, NTV) hipLaunchKernelGGL((csr_stream_kernel<T, FUSED, C16V, NTV>), dim3(gx), dim3(HIPK_BLOCK), 0, st, \
      A->tileinfo, A->ntiles, A->rowptr, A->colind, rt.c16 ? A->col16 : (const uint16_t *)NULL, A->row0 - A->c16back, (const T *)A->values, \
      x, ldx, y, ldy, 1, A->x0, A->xlen, A->halo_lo, A->halo_hi, (const T *)A->xlo, (const T *)A->xhi, A->ld_lo, A->ld_hi, norm2, xout, partials, fa)
   if (rt.nt) { if (rt.c16) LAUNCH_STREAM(true, true); else LAUNCH_STREAM(false, true); }
   else { if (rt.c16) LAUNCH_STREAM(true, false); else LAUNCH_STREAM(false, false); }
#undef LAUNCH_STREAM
}

template <typename T>
void csr_launch_scaled(const hipk_csr *A, const csr_route &rt, hipStream_t st, int gx, const T *x, const double *norm2, T *xout, T *y,
      double *partials, const hipk_fin_args &fa) {
   launch_stream<T, true>(A, rt, st, gx, x, A->nrows, y, A->nrows, norm2, xout, partials, fa);
}

template <typename T>
void csr_launch_tiles(const hipk_csr *A, const csr_route &rt, hipStream_t st, const T *x, int64_t ldx, T *y, int64_t ldy, int ncols,
      const double *shift_host, const SpmmCheb<T> *cheb) {
   const int gx = ((A->ntiles + 7) / 8) * 8;
   if (rt.kernel == CSR_K_STREAM) {
      launch_stream<T, false>(A, rt, st, gx, x, ldx, y, ldy, (const double *)NULL, (T *)NULL, (double *)NULL, hipk_fin_args());
   } else if (rt.kernel == CSR_K_ROWS) {
#define LAUNCH_ROWS(NCV) hipLaunchKernelGGL((csr_rows_block_kernel<T, NCV>), dim3(gx), dim3(HIPK_BLOCK), 0, st, \
      A->tiles, A->ntiles, A->rowptr, A->colind, (const T *)A->values, x, ldx, y, ldy, \
      ncols, A->x0, A->xlen, A->halo_lo, A->halo_hi, (const T *)A->xlo, (const T *)A->xhi, A->ld_lo, A->ld_hi)
      if (rt.nc == 1) LAUNCH_ROWS(1); else if (rt.nc == 2) LAUNCH_ROWS(2); else LAUNCH_ROWS(4);
#undef LAUNCH_ROWS
   } else {
      SpmmShift sh;
      sh.on = shift_host != NULL;
      sh.nosplit = csr_knobs().no_split || (cheb && cheb->seq < 0);
      sh.evenstride = csr_knobs().even_stride;
      for (int c = 0; c < 64; c++) sh.s[c] = (shift_host && c < ncols) ? shift_host[c] : 0.0;
      /* the window buffer in two sizes: XS_SMALL values when every window of this matrix fits (4 workgroups per CU) and
       * XS_MAX otherwise (50 KB of LDS, 3 per CU) */
#define LAUNCH_WIN_ARGS A->tileinfo, A->twin, A->ntiles, A->rowptr, A->colind, rt.c16 ? A->col16 : (const uint16_t *)NULL, A->row0 - A->c16back, \
      (const T *)A->values, x, ldx, y, ldy, ncols, A->x0, sh
#define LAUNCH_WIN(NCV, XSV, C16V) do { \
      if (cheb) hipLaunchKernelGGL((csr_window_block_kernel<T, NCV, XSV, C16V, true>), dim3(gx), dim3(HIPK_BLOCK), 0, st, LAUNCH_WIN_ARGS, *cheb); \
      else hipLaunchKernelGGL((csr_window_block_kernel<T, NCV, XSV, C16V, false>), dim3(gx), dim3(HIPK_BLOCK), 0, st, LAUNCH_WIN_ARGS, SpmmNoEp()); } while (0)
#define LAUNCH_WIN2(NCV, XSV) do { if (rt.c16) LAUNCH_WIN(NCV, XSV, true); else LAUNCH_WIN(NCV, XSV, false); } while (0)
      if (rt.nc == 2) { if (rt.xs_small) LAUNCH_WIN2(2, XS_SMALL); else LAUNCH_WIN2(2, XS_MAX); }
      else { if (rt.xs_small) LAUNCH_WIN2(4, XS_SMALL); else LAUNCH_WIN2(4, XS_MAX); }
#undef LAUNCH_WIN2
#undef LAUNCH_WIN
#undef LAUNCH_WIN_ARGS
   }
}

#define CSR_LAUNCHERS(T) \
   template void csr_launch_stencil<T>(const hipk_csr *, hipStream_t, const T *, int64_t, T *, int64_t, int); \
   template void csr_launch_tiles<T>(const hipk_csr *, const csr_route &, hipStream_t, const T *, int64_t, T *, int64_t, int, const double *, const SpmmCheb<T> *); \
   template void csr_launch_scaled<T>(const hipk_csr *, const csr_route &, hipStream_t, int, const T *, const double *, T *, T *, double *, const hipk_fin_args &);
CSR_LAUNCHERS(double)
CSR_LAUNCHERS(float)
