/* hipk_sparse_dev.h — what the row-tile kernels (hipk_sparse.hip) and the hipk_csr object (hipk_csr.hip) share: the
 * object, the routing record that says which form and kernel serve a product, the launchers' prototypes, and the device
 * code the tile kernels have in common.  Included by .hip files only. */
#ifndef HIPK_SPARSE_DEV_H
#define HIPK_SPARSE_DEV_H

#include "hipk_internal.h"
#include "primme_amd_io.h"

/* the limits of the host's tile plan (csr_tools.c: primme_amd_csr_tile_plan) are the sizes of the kernels' LDS arrays */
#define TILE_NNZ PRIMME_AMD_TILE_NNZ
#define TILE_ROWS PRIMME_AMD_TILE_ROWS
#define XS_MAX PRIMME_AMD_TILE_WINDOW
#define XS_SMALL 1728      /* 192 window rows of 8 columns on the odd stride of 9: 39 KB of LDS per workgroup, still 4 per CU (1536 until round 6) */
#define TILE_PER_LANE (TILE_NNZ / HIPK_BLOCK)   /* nonzeros a lane handles per tile */

struct hipk_csr {
   hipk_ctx *ctx;
   hipk_dtype dt;
   int kind;               /* 0 = CSR, 1 = stencil */
   int64_t nrows, ncols_global, row0, nnz;
   int64_t x0, xlen;       /* entries [x0, x0+xlen) of the input vector are owned (= the row slab for
                              square row-partitioned operators, everything for rectangular ones) */
   int32_t *rowptr, *colind;   /* device */
   void *values;               /* device */
   int32_t *tiles;             /* device: ntiles+1 row offsets */
   int4 *tileinfo;             /* device: {first row, end row, first nonzero, end nonzero} per tile */
   int2 *twin;                 /* device: {first column, window width} per tile; width 0 = not windowable */
   uint16_t *col16;            /* device, or NULL: column - (row0 + first row of the tile - c16back) for every nonzero, when that
                                  fits 16 bits for the whole matrix (banded / stencil / block-diagonal patterns): 2 bytes per
                                  nonzero out of HBM instead of 4 in the tile kernels, the base follows from the tile record */
   int64_t c16back;            /* how far below its first row a tile's columns reach, at most */
   int windowed;               /* most tiles have a narrow column window inside the owned slab */
   int cw_max;                 /* widest window among the windowable tiles */
   int ntiles;
   void *diag;                 /* device, nrows elements */
   int64_t halo_lo, halo_hi;   /* extent of off-rank columns below / above */
   const void *xlo, *xhi;      /* device halo buffers for the current matvec */
   int64_t ld_lo, ld_hi;       /* their column strides (default: halo_lo / halo_hi, packed) */
   int sx, sy, sz;             /* stencil grid */
   struct hipk_pb *pb;         /* panel-blocked form (hipk_sparse_pb.hip) for scattered column patterns, or NULL */
   struct hipk_pat *pat;       /* row-pattern dictionary form (hipk_sparse_pat.hip) for matrices whose rows repeat, or NULL */
   struct hipk_sell *sell;     /* sliced-ELL form (hipk_sparse_sell.hip), built on request (HIPK_CSR_SLICED) beside the CSR arrays, or NULL */
};

/* Which form and kernel serve a product, and the bytes it moves: csr_route (hipk_csr.hip) decides, everything else switches
 * on the record.  The forms carry the numbers hipk_csr_format returns. */
enum { CSR_TILES = 0, CSR_PB = 1, CSR_PAT = 2, CSR_STENCIL = 3, CSR_SELL = 4 };
enum { CSR_OP_PLAIN, CSR_OP_SHIFTED, CSR_OP_CHEB, CSR_OP_CHEB_GATHER, CSR_OP_SCALED };      /* the kinds of product */
enum { CSR_K_STREAM, CSR_K_ROWS, CSR_K_WINDOW };                                              /* the row-tile kernels */
struct csr_route {
   int own;                /* the form that holds this matrix' one-column products right now (hipk_csr_format) */
   int form;               /* the form that serves THIS product: `own`, or the row tiles when `own` does not cover it */
   int kernel;             /* row tiles: csr_stream_kernel / csr_rows_block_kernel / csr_window_block_kernel ... */
   int nc, xs_small, c16, nt;      /* ... and its variant: columns per lane, the small window buffer, the 2-byte index stream, non-temporal loads */
   int index_bytes;        /* bytes per nonzero that kernel reads for the column */
   double alg, streamed;   /* algorithmic bytes of the product, and what the form in use really moves (a Chebyshev step's
                              other panels not counted: the caller knows which it was given) */
};
csr_route csr_route_of(const hipk_csr *A, int ncols, int op);

/* The A/B and measurement knobs of the CSR products, read from the environment once (csr_knobs, hipk_csr.hip) */
struct csr_knob_set {
   int nc;                 /* HIPK_SPMM_NC=1|2|4: always csr_rows_block_kernel with that many columns per lane (0: by width) */
   int no_window;          /* HIPK_NO_WINDOW: plain products never take the windowed kernel */
   int no_split;           /* HIPK_SPMM_NO_SPLIT: one lane per row always in the windowed kernel */
   int even_stride;        /* HIPK_SPMM_EVEN_STRIDE: window rows ncols apart in LDS, as until round 5 */
   int big_window;         /* HIPK_SPMM_BIG_WINDOW: always the large window buffer */
   int no_col16;           /* HIPK_SPMM_NO_COL16: never the 2-byte index stream */
   int nt;                 /* HIPK_SPMV_NT=0|1: never / always stream the matrix past the Infinity Cache (-1: by its size) */
   int pb_maxcols;         /* HIPK_PB_MAXCOLS: widest block served column by column through the panel-blocked form (2) */
};
const csr_knob_set &csr_knobs(void);

/* CHEB: the row sums are not stored but combined with the row's own entries of up to three panels — one step of the Chebyshev
 * recurrence (hipk_cheb.hip): y(i,c) = cy[c] yk(i,c) + cp[c] yp(i,c) + cx[c] xr(i,c) + cw[c] (A x)(i,c).  Square operators
 * (hipk_csr_cheb_step): yk is x, the iterate the product gathers from.  Rectangular ones (hipk_csr_cheb_step_gather): x has
 * ncols(A) rows and is only gathered, yk is a panel of its own or NULL; yp == NULL: no such term.  y may be yk or yp (row-local),
 * never x.  seq: the row sum of a one-column call is formed as csr_stream_kernel forms it (every product rounded, then added in
 * row order, one lane per row), so that the step equals that kernel followed by cheb_update_kernel bit for bit. */
template <typename T> struct SpmmCheb { hipk_cheb_coef cf; const T *xr; int64_t ldr; const T *yp; int64_t ldp; const T *yk; int64_t ldk; int seq; };

/* the launchers of hipk_sparse.hip (T = double, float): the stencil, the row-tile kernel `rt` names, the fused one-column product */
template <typename T> void csr_launch_stencil(const hipk_csr *A, hipStream_t st, const T *x, int64_t ldx, T *y, int64_t ldy, int ncols);
template <typename T> void csr_launch_tiles(const hipk_csr *A, const csr_route &rt, hipStream_t st, const T *x, int64_t ldx, T *y, int64_t ldy,
      int ncols, const double *shift_host, const SpmmCheb<T> *cheb);
template <typename T> void csr_launch_scaled(const hipk_csr *A, const csr_route &rt, hipStream_t st, int gx, const T *x, const double *norm2,
      T *xout, T *y, double *partials, const hipk_fin_args &fa);

/* x element for global column g: owned slab, or the lo / hi halo buffers.  The address is
 * selected, the load itself is unconditional (a branch per gather would serialise the gathers). */
template <typename T>
__device__ __forceinline__ double fetch_x(const T *__restrict__ x, const T *__restrict__ xlo,
      const T *__restrict__ xhi, int64_t row0, int64_t nrows, int64_t halo_lo, int64_t g) {
   const int64_t l = g - row0;
   const T *p = x + l;
   if (l < 0) p = xlo + (l + halo_lo);
   if (l >= nrows) p = xhi + (l - nrows);
   return (double)*p;
}

/* XCD-aware tile order: block b -> tile ((b % 8) * per + b / 8) so that each XCD
 * (blocks are dealt round-robin to the 8 XCDs) owns a contiguous range of tiles. */
__device__ __forceinline__ int xcd_tile(int b, int ntiles) {
   const int per = (ntiles + 7) >> 3;
   return (b & 7) * per + (b >> 3);
}

/* This lane's (value, column) loads of a tile of nz <= TILE_NNZ nonzeros at p0, all in flight at once: indices clamped, not
 * predicated, so nothing branches around a load (an all-empty tile reads the padded element).  C16: the 2-byte entry, raw. */
template <typename T, bool C16>
__device__ __forceinline__ void csr_tile_loads(const T *__restrict__ val, const int32_t *__restrict__ colind, const uint16_t *__restrict__ col16,
      int p0, int nz, T (&tv)[TILE_PER_LANE], int32_t (&tc)[TILE_PER_LANE]) {
#pragma unroll
   for (int u = 0; u < TILE_PER_LANE; u++) {
      const int q = threadIdx.x + u * HIPK_BLOCK;
      const int qc = q < nz ? q : (nz > 0 ? nz - 1 : 0);
      tv[u] = val[p0 + qc];
      if (C16) tc[u] = (int32_t)col16[p0 + qc];
      else tc[u] = colind[p0 + qc];
   }
}

#endif
