/* primme_amd_io.h — C-ABI of the host-side matrix ingest: the on-disk
 * format and the tiler either side of the hot path.
 *
 *   primme_amd_mm_read   replaces what the reference's test driver does with
 *                        tests/COMMON/mmio.c:27-316 and tests/COMMON/csr.c:98-239 (readfullMTX):
 *                        Matrix-Market coordinate file -> CSR with sorted rows, expanding
 *                        symmetric / Hermitian / skew-symmetric storage
 *   primme_amd_csr_tile_block_diagonal   block-diagonal tiling, tile t scaled by
 *                        scale0 + scale_step * t (BASELINE configs[2] from tests/LUNDA.mtx)
 *   primme_amd_csr_transpose             explicit transpose (singular value operator)
 *   primme_amd_csr_complex_to_real       2n x 2n real-equivalent form of a complex matrix in the
 *                        interleaved (re, im) ordering: the operator hip_zprimme / hip_cprimme
 *                        are given for a Hermitian CSR matrix (primme_amd.h)
 *   primme_amd_csr_row_patterns_diag     the scan of the diagonal-split row-pattern form of the device operator
 *                        (primme_amd_kernels.h: HIPK_CSR_DIAG_PATTERNS): rows [row0, row0 + m) as one byte per row
 *                        (pid[m + 1]) + a table of npat <= 256 patterns of stride ml (3/5/7/8): len[npat],
 *                        off[npat * ml] = column - row, val[npat * ml] (0 at the diagonal's place) and dslot[npat], the
 *                        index of the entry with offset 0 or -1.  values: double, or float when is_float.  Returns 1
 *                        (nothing allocated) when the matrix does not qualify: a row longer than 8, a 257th pattern,
 *                        two diagonal entries in a row, offsets out of reach
 *
 *   primme_amd_csr_to_sliced             the sliced-ELL form (SELL-64-256) of the device operator created with HIPK_CSR_SLICED;
 *                        layout at its declaration below
 *   primme_amd_csr_tile_plan             the host analysis of the device CSR operator's row-tile kernels: tiles, column
 *                        windows, halo extent, diagonal and the 16-bit index stream; fields at its declaration below
 *
 * 0-based int32 indices; values double (complex: re, im interleaved).  Returned arrays are
 * malloc'ed by the library: release them with primme_amd_host_free.  Return 0 on success,
 * -1 cannot open, -2 malformed, -3 unsupported variant, -4 too large for int32, -5 out of memory. */
#ifndef PRIMME_AMD_IO_H
#define PRIMME_AMD_IO_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int primme_amd_mm_read(const char *path, int64_t *m, int64_t *n, int64_t *nnz, int32_t **rowptr,
      int32_t **colind, double **values, int *is_complex);
int primme_amd_csr_transpose(int64_t m, int64_t n, const int32_t *rowptr, const int32_t *colind,
      const void *values, size_t elem_size, int32_t **rowptrT, int32_t **colindT, void **valuesT);
int primme_amd_csr_tile_block_diagonal(int64_t n0, const int32_t *rowptr, const int32_t *colind,
      const double *values, int64_t ntiles, int64_t first_tile, double scale0, double scale_step,
      int32_t **rowptr_out, int32_t **colind_out, double **values_out);
int primme_amd_csr_complex_to_real(int64_t n, const int32_t *rowptr, const int32_t *colind,
      const double *values_re_im, int32_t **rowptr_out, int32_t **colind_out, double **values_out);
int primme_amd_csr_row_patterns_diag(int64_t m, int64_t row0, const int32_t *rowptr, const int32_t *colind,
      const void *values, int is_float, uint8_t **pid, int *npat, int *ml, int32_t **len, int32_t **off,
      double **val, int32_t **dslot);
/* Sliced-ELL form of a CSR matrix, SELL-64-256: what the device operator keeps beside the CSR arrays when it is created with
 * HIPK_CSR_SLICED (primme_amd_kernels.h).
 *   windows  256 consecutive rows; the rows of a window are sorted by descending length (stable) and become its SLOTS;
 *            slot p of the matrix (window p / 256) holds row (p / 256) * 256 + perm[p] and that row's length len[p]
 *   slices   64 consecutive slots; nslices = ceil(m / 64), the last window and the last slice may be ragged (slots >= m
 *            have length 0).  Slice s is as wide as its longest row, width_s = (base[s + 1] - base[s]) / 64, and stores
 *            entry j of its slot l at base[s] + 64 j + l: a row's entries in their CSR order, then padding
 *   columns  idx16 = 1 (every slice's columns span less than 65 536): uint16 entries, column = cmin[s] + entry;
 *            idx16 = 0: int32 entries, the columns themselves (cmin[s] = 0).  One width per matrix
 *   padding  value 0 and a column some row of the matrix references; a product must skip it by the row's length (0 * x is
 *            not 0 when x is NaN or Inf)
 *   padded   sum over the slices of width_s * (slots of the slice that exist): the entries a product reads.  The form is
 *            built when padded <= max_padding * nnz (the device operator asks for 1.25); the arrays hold base[nslices]
 *            entries, the ragged last slice allocated 64 wide
 * values: elem_size bytes each, copied bit for bit.  Returns 0 and *S (release with primme_amd_sliced_free), 1 when the
 * padding is above the limit or the matrix has no entry (nothing allocated), -4 a row longer than 65 535, -5 out of memory. */
typedef struct primme_amd_sliced {
   int64_t m, nnz, nslices, padded;
   int idx16;
   int64_t *base;        /* nslices + 1 */
   int32_t *cmin;        /* nslices */
   uint8_t *perm;        /* 64 nslices */
   uint16_t *len;        /* 64 nslices */
   void *val;            /* base[nslices] elements */
   void *idx;            /* base[nslices] uint16 / int32 */
} primme_amd_sliced;
int primme_amd_csr_to_sliced(int64_t m, const int32_t *rowptr, const int32_t *colind, const void *values, size_t elem_size,
      double max_padding, primme_amd_sliced **S);
void primme_amd_sliced_free(primme_amd_sliced *S);
/* Row tiles of the device CSR operator (hipk_csr_create*): what its tile kernels are launched over.  The limits are shared
 * with the kernels: a tile holds at most PRIMME_AMD_TILE_NNZ nonzeros and PRIMME_AMD_TILE_ROWS consecutive rows (greedy; a
 * single longer row is a tile of its own), a column window at most PRIMME_AMD_TILE_WINDOW columns.
 *   rows [row0, row0 + nrows) of the matrix; entries [x0, x0 + xlen) of the input vector are owned, others are halo
 *   tiles    ntiles + 1 row offsets;  info: {first row, end row, first nonzero, end nonzero} per tile;  win: {first column,
 *            width} of the tile's columns when they lie inside the owned entries and span at most the window limit, else
 *            {0, 0}.  info and win hold one more, zero, record
 *   cw_max   the widest window;  windowed: no halo and at least 9 tiles in 10 have a window with 8 width <= the limit
 *   halo_lo / halo_hi   how far the columns reach below x0 / beyond x0 + xlen;  diag: the entry at column row0 + i of
 *            row i (0 without one), nrows elements of elem_size bytes
 *   col16    real_values only, else NULL: column - (row0 + first row of the tile - c16back) for every nonzero (+ one zero
 *            entry), c16back = the farthest a tile's columns reach below its first row; NULL when an entry would exceed
 *            65 535 or row0 - c16back / ncols_global leave the int32 range the kernels compute in
 * Returns 0 and *P (release with primme_amd_tile_plan_free), -5 out of memory. */
#define PRIMME_AMD_TILE_NNZ 2048
#define PRIMME_AMD_TILE_ROWS 256
#define PRIMME_AMD_TILE_WINDOW 3072
typedef struct primme_amd_tile_plan {
   int ntiles, cw_max, windowed;
   int64_t halo_lo, halo_hi, c16back;
   int32_t *tiles;       /* ntiles + 1 */
   int32_t *info;        /* 4 (ntiles + 1) */
   int32_t *win;         /* 2 (ntiles + 1) */
   void *diag;           /* nrows elements */
   uint16_t *col16;      /* nnz + 1, or NULL */
} primme_amd_tile_plan;
int primme_amd_csr_tile_plan(int64_t nrows, int64_t row0, int64_t x0, int64_t xlen, int64_t ncols_global, const int32_t *rowptr,
      const int32_t *colind, const void *values, size_t elem_size, int real_values, primme_amd_tile_plan **P);
void primme_amd_tile_plan_free(primme_amd_tile_plan *P);
/* Hierarchy of the aggregation algebraic multigrid preconditioner (primme_amd_amg_precond in primme_amd.h; DESIGN.md
 * section 4o), built on the host from the CSR arrays of a SYMMETRIC matrix A with a positive diagonal: symmetry is the caller's
 * promise and is not checked.  values: elem_size 8 (double) or 4 (float).  Level 0 is M_0 = A + shift I; level l + 1 is the
 * Galerkin matrix M_{l+1} = P_l' M_l P_l of plain (unsmoothed) aggregation, P_l the 0/1 matrix of agg_l, summed in double with
 * sorted columns and one entry per position.
 *   strong   i ~ j (i != j) when |m_ij| >= theta sqrt(m_ii m_jj)
 *   pass 1   rows in index order: a free row whose strong neighbours are all free founds an aggregate with them
 *   pass 2   rows in index order: a free row joins the pass-1 aggregate it has the largest strong |m_ij| to (ties: the lowest
 *            aggregate number); rows that joined in this pass attract nobody
 *   pass 3   rows in index order: a row still free founds an aggregate with its free strong neighbours (maybe alone)
 * The result depends on the matrix alone.  Level l is the last when n_l <= PRIMME_AMD_AMG_DENSE_ROWS, when it is level
 * PRIMME_AMD_AMG_MAXLEVELS - 1, or when the aggregation would keep more than 0.8 n_l rows (the aggregation is then discarded).
 * Per level: n rows, the CSR arrays of M_l, dinv = 1 / diag(M_l), rho = max_i sum_j |m_ij| / m_ii (a bound on the spectrum
 * of D^-1 M_l) and, but on the last level (nc = 0, NULL), the aggregate map agg[n] with values in [0, nc) and its inverse:
 * aggregate j holds the rows aggrows[aggptr[j] .. aggptr[j + 1]), ascending.
 * primme_amd_amg_plan_create returns 0 and *plan (release with primme_amd_amg_plan_free), -1 for n < 1, theta outside [0, 1),
 * shift < 0, a row without a diagonal entry or a diagonal entry <= 0 on any level, -4 beyond int32, -5 out of memory.
 * primme_amd_amg_coarse_inverse writes G = M_L^-1 (n_L x n_L, symmetric, n_L <= PRIMME_AMD_AMG_DENSE_ROWS) of the last
 * level from a Cholesky factorisation; -1 when M_L is not positive definite or has more rows.
 *
 * primme_amd_amg_plan_create_smoothed builds the hierarchy of SMOOTHED aggregation with the same
 * aggregation passes, stop rules, per-level data and error returns.  T_l being the 0/1 matrix of agg_l,
 *    P_l = (I - (omega / rho_l) D_l^-1 M_l) T_l         (M_l unfiltered, the columns of T_l not normalised)
 *    M_{l+1} = P_l' M_l P_l                             (a general sparse triple product in double)
 * with sorted columns and one entry per position in both; the upper triangle of M_{l+1} is computed and mirrored, so it is
 * exactly symmetric.  transfer[l] of every level but the last holds P_l in CSR (n_l rows, pnnz entries) and its explicit
 * transpose R_l = P_l' in CSR (nc_l rows, ascending columns, the values the same bits); the plain plan leaves transfer[] NULL
 * and omega 0.  omega in (0, 2), 4/3 the usual choice; outside: -1.  -4 also when nnz(P_l) or nnz(M_{l+1}) passes int32. */
#define PRIMME_AMD_AMG_MAXLEVELS 24
#define PRIMME_AMD_AMG_DENSE_ROWS 256
typedef struct primme_amd_amg_level {
   int64_t n, nnz, nc;
   int32_t *rowptr, *colind;
   double *values, *dinv;
   double rho;
   int32_t *agg, *aggptr, *aggrows;
} primme_amd_amg_level;
typedef struct primme_amd_amg_transfer {
   int64_t pnnz;
   int32_t *prowptr, *pcolind;   /* P_l: n + 1, pnnz */
   double *pvalues;
   int32_t *rrowptr, *rcolind;   /* R_l = P_l': nc + 1, pnnz */
   double *rvalues;
} primme_amd_amg_transfer;
typedef struct primme_amd_amg_plan {
   int nlevels;
   double shift, theta;
   primme_amd_amg_level level[PRIMME_AMD_AMG_MAXLEVELS];
   double omega;                 /* 0: plain aggregation */
   primme_amd_amg_transfer transfer[PRIMME_AMD_AMG_MAXLEVELS];
} primme_amd_amg_plan;
int primme_amd_amg_plan_create(int64_t n, const int32_t *rowptr, const int32_t *colind, const void *values, size_t elem_size,
      double shift, double theta, primme_amd_amg_plan **plan);
int primme_amd_amg_plan_create_smoothed(int64_t n, const int32_t *rowptr, const int32_t *colind, const void *values, size_t elem_size,
      double shift, double theta, double omega, primme_amd_amg_plan **plan);
void primme_amd_amg_plan_free(primme_amd_amg_plan *plan);
int primme_amd_amg_coarse_inverse(const primme_amd_amg_plan *plan, double *G);
void primme_amd_host_free(void *p);
#ifdef __cplusplus
}
#endif
#endif
