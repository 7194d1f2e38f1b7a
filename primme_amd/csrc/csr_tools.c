/* csr_tools.c — host-side matrix ingest feeding the device operators.
 *
 *   primme_amd_mm_read            <- reference tests/COMMON/mmio.c:27-316 (banner / size parsing)
 *                                    + tests/COMMON/csr.c:98-239 (readfullMTX: COO -> CSR,
 *                                    symmetric / Hermitian / skew expansion, sorted rows)
 *   primme_amd_csr_tile_block_diagonal  the tiler that builds BASELINE configs[2] from LUNDA.mtx
 *   primme_amd_csr_transpose      explicit A' for the singular value operator
 *   primme_amd_csr_complex_to_real  Hermitian matrix -> symmetric real-equivalent form
 *   primme_amd_csr_tile_plan      the row tiles, column windows and 16-bit index stream of the device CSR operator
 *   primme_amd_mg_plan            the grids and weights of the geometric multigrid preconditioner (primme_amd.h)
 *   primme_amd_amg_plan_create    the aggregates and Galerkin matrices of the algebraic multigrid preconditioner
 *   primme_amd_amg_plan_create_smoothed   the same with smoothed prolongations and a general triple product
 *
 * Indices are 0-based int32 (the device kernels' format); values are double, complex as
 * (re, im) pairs.  Everything returned is malloc'ed; release with primme_amd_host_free. */
#include <ctype.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "primme_amd_io.h"
#include "primme_amd.h"
#include "amg_internal.h"

void primme_amd_host_free(void *p) { free(p); }

typedef struct { int32_t r, c; double re, im; } coo_t;
static int coo_cmp(const void *a, const void *b) {
   const coo_t *x = (const coo_t *)a, *y = (const coo_t *)b;
   if (x->r != y->r) return x->r < y->r ? -1 : 1;
   if (x->c != y->c) return x->c < y->c ? -1 : 1;
   return 0;
}

static void lower(char *s) { for (; *s; s++) *s = (char)tolower((unsigned char)*s); }

int primme_amd_mm_read(const char *path, int64_t *m_out, int64_t *n_out, int64_t *nnz_out,
      int32_t **rowptr_out, int32_t **colind_out, double **values_out, int *is_complex_out) {
   FILE *f = fopen(path, "r");
   if (!f) return -1;
   char line[1100], banner[64], object[64], format[64], field[64], symmetry[64];
   if (!fgets(line, sizeof line, f)) { fclose(f); return -2; }
   if (sscanf(line, "%63s %63s %63s %63s %63s", banner, object, format, field, symmetry) != 5) { fclose(f); return -2; }
   lower(object); lower(format); lower(field); lower(symmetry);
   if (strcmp(banner, "%%MatrixMarket") != 0 || strcmp(object, "matrix") != 0) { fclose(f); return -2; }
   if (strcmp(format, "coordinate") != 0) { fclose(f); return -3; }    /* dense arrays: not an operator file */
   const int pattern = !strcmp(field, "pattern"), cplx = !strcmp(field, "complex");
   if (!pattern && !cplx && strcmp(field, "real") != 0 && strcmp(field, "integer") != 0) { fclose(f); return -3; }
   const int sym = !strcmp(symmetry, "symmetric"), herm = !strcmp(symmetry, "hermitian"),
             skew = !strcmp(symmetry, "skew-symmetric");
   if (!sym && !herm && !skew && strcmp(symmetry, "general") != 0) { fclose(f); return -3; }

   do {
      if (!fgets(line, sizeof line, f)) { fclose(f); return -2; }
   } while (line[0] == '%' || line[0] == '\n' || line[0] == '\r');
   long long m, n, nz;
   if (sscanf(line, "%lld %lld %lld", &m, &n, &nz) != 3 || m < 0 || n < 0 || nz < 0) { fclose(f); return -2; }
   if (m >= 2147483647LL || n >= 2147483647LL) { fclose(f); return -4; }

   const int expand = sym || herm || skew;
   coo_t *e = (coo_t *)malloc(sizeof(coo_t) * (size_t)(expand ? 2 * nz : nz) + sizeof(coo_t));
   if (!e) { fclose(f); return -5; }
   long long cnt = 0;
   for (long long k = 0; k < nz; k++) {
      long long i, j;
      double re = 1.0, im = 0.0;
      int got;
      if (pattern) got = fscanf(f, "%lld %lld", &i, &j) == 2;
      else if (cplx) got = fscanf(f, "%lld %lld %lf %lf", &i, &j, &re, &im) == 4;
      else got = fscanf(f, "%lld %lld %lf", &i, &j, &re) == 3;
      if (!got || i < 1 || j < 1 || i > m || j > n) { free(e); fclose(f); return -2; }
      e[cnt].r = (int32_t)(i - 1); e[cnt].c = (int32_t)(j - 1); e[cnt].re = re; e[cnt].im = im; cnt++;
      if (expand && i != j) {
         e[cnt].r = (int32_t)(j - 1); e[cnt].c = (int32_t)(i - 1);
         e[cnt].re = skew ? -re : re;
         e[cnt].im = herm ? -im : (skew ? -im : im);
         cnt++;
      }
   }
   fclose(f);
   if (cnt >= 2147483647LL) { free(e); return -4; }
   qsort(e, (size_t)cnt, sizeof(coo_t), coo_cmp);

   int32_t *rp = (int32_t *)calloc((size_t)m + 1, sizeof(int32_t));
   int32_t *ci = (int32_t *)malloc(sizeof(int32_t) * (size_t)(cnt > 0 ? cnt : 1));
   double *va = (double *)malloc(sizeof(double) * (size_t)(cnt > 0 ? cnt : 1) * (cplx ? 2 : 1));
   if (!rp || !ci || !va) { free(e); free(rp); free(ci); free(va); return -5; }
   for (long long k = 0; k < cnt; k++) {
      rp[e[k].r + 1]++;
      ci[k] = e[k].c;
      if (cplx) { va[2 * k] = e[k].re; va[2 * k + 1] = e[k].im; } else va[k] = e[k].re;
   }
   for (long long i = 0; i < m; i++) rp[i + 1] += rp[i];
   free(e);
   *m_out = m; *n_out = n; *nnz_out = cnt;
   *rowptr_out = rp; *colind_out = ci; *values_out = va; *is_complex_out = cplx;
   return 0;
}

int primme_amd_csr_transpose(int64_t m, int64_t n, const int32_t *rp, const int32_t *ci, const void *val,
      size_t elem_size, int32_t **rpT_out, int32_t **ciT_out, void **valT_out) {
   const int64_t nnz = rp[m];
   int32_t *rpT = (int32_t *)calloc((size_t)n + 2, sizeof(int32_t));
   int32_t *ciT = (int32_t *)malloc(sizeof(int32_t) * (size_t)(nnz > 0 ? nnz : 1));
   char *vT = (char *)malloc(elem_size * (size_t)(nnz > 0 ? nnz : 1));
   if (!rpT || !ciT || !vT) { free(rpT); free(ciT); free(vT); return -5; }
   for (int64_t k = 0; k < nnz; k++) rpT[ci[k] + 2]++;
   for (int64_t j = 0; j < n; j++) rpT[j + 2] += rpT[j + 1];
   /* rpT[j+1] is now the insertion cursor of column j; rows visited in order keep A' sorted */
   for (int64_t i = 0; i < m; i++)
      for (int32_t k = rp[i]; k < rp[i + 1]; k++) {
         const int32_t dst = rpT[ci[k] + 1]++;
         ciT[dst] = (int32_t)i;
         memcpy(vT + (size_t)dst * elem_size, (const char *)val + (size_t)k * elem_size, elem_size);
      }
   *rpT_out = rpT; *ciT_out = ciT; *valT_out = vT;
   return 0;
}

int primme_amd_csr_tile_block_diagonal(int64_t n0, const int32_t *rp, const int32_t *ci, const double *val,
      int64_t ntiles, int64_t first_tile, double scale0, double scale_step, int32_t **rp_out,
      int32_t **ci_out, double **val_out) {
   const int64_t nnz0 = rp[n0];
   if (n0 * (first_tile + ntiles) >= 2147483647LL || nnz0 * ntiles >= 2147483647LL) return -4;
   int32_t *trp = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n0 * ntiles + 1));
   int32_t *tci = (int32_t *)malloc(sizeof(int32_t) * (size_t)(nnz0 * ntiles > 0 ? nnz0 * ntiles : 1));
   double *tva = (double *)malloc(sizeof(double) * (size_t)(nnz0 * ntiles > 0 ? nnz0 * ntiles : 1));
   if (!trp || !tci || !tva) { free(trp); free(tci); free(tva); return -5; }
   trp[0] = 0;
   for (int64_t t = 0; t < ntiles; t++) {
      const double s = scale0 + scale_step * (double)(first_tile + t);
      const int64_t coff = (first_tile + t) * n0;
      for (int64_t i = 0; i < n0; i++) trp[t * n0 + i + 1] = (int32_t)(rp[i + 1] + t * nnz0);
      for (int64_t k = 0; k < nnz0; k++) {
         tci[t * nnz0 + k] = (int32_t)(ci[k] + coff);
         tva[t * nnz0 + k] = val[k] * s;
      }
   }
   *rp_out = trp; *ci_out = tci; *val_out = tva;
   return 0;
}

/* Real-equivalent form of a complex CSR matrix in the interleaved ordering: entry a + ib at
 * (i, j) becomes the 2x2 block [a -b; b a] at rows 2i, 2i+1 and columns 2j, 2j+1, so that the
 * 2n real vector (re0, im0, re1, im1, ...) -- the memory of the complex n-vector -- is mapped to
 * the memory of A x.  A Hermitian gives a symmetric matrix whose eigenvalues are those of A, each
 * twice (eigs_complex.c).  values: (re, im) pairs of double. */
int primme_amd_csr_complex_to_real(int64_t n, const int32_t *rp, const int32_t *ci, const double *val,
      int32_t **rp_out, int32_t **ci_out, double **val_out) {
   const int64_t nnz = rp[n];
   if (2 * n >= 2147483647LL || 4 * nnz >= 2147483647LL) return -4;
   int32_t *rp2 = (int32_t *)malloc(sizeof(int32_t) * (size_t)(2 * n + 1));
   int32_t *ci2 = (int32_t *)malloc(sizeof(int32_t) * (size_t)(4 * nnz > 0 ? 4 * nnz : 1));
   double *va2 = (double *)malloc(sizeof(double) * (size_t)(4 * nnz > 0 ? 4 * nnz : 1));
   if (!rp2 || !ci2 || !va2) { free(rp2); free(ci2); free(va2); return -5; }
   int64_t o = 0;
   rp2[0] = 0;
   for (int64_t i = 0; i < n; i++) {
      for (int32_t k = rp[i]; k < rp[i + 1]; k++) {   /* row 2i: (a, -b) */
         ci2[o] = 2 * ci[k];     va2[o++] = val[2 * (size_t)k];
         ci2[o] = 2 * ci[k] + 1; va2[o++] = -val[2 * (size_t)k + 1];
      }
      rp2[2 * i + 1] = (int32_t)o;
      for (int32_t k = rp[i]; k < rp[i + 1]; k++) {   /* row 2i+1: (b, a) */
         ci2[o] = 2 * ci[k];     va2[o++] = val[2 * (size_t)k + 1];
         ci2[o] = 2 * ci[k] + 1; va2[o++] = val[2 * (size_t)k];
      }
      rp2[2 * i + 2] = (int32_t)o;
   }
   *rp_out = rp2; *ci_out = ci2; *val_out = va2;
   return 0;
}

/* Diagonal-split row patterns (device/hipk_sparse_pat.hip): a row's pattern is its length, its (column - row) offsets, its
 * OFF-DIAGONAL values and the position of the entry with offset 0 (dslot, -1: the row stores no diagonal); the diagonal's
 * value is not part of the pattern (the table holds 0 there) — the kernel reads it per row.  "-Laplacian + potential" has the
 * patterns of the Laplacian.  Values enter the table as (double)(T) of the stored value, T = float when is_float.
 * Returns 0 and pid[m + 1] (pid[m] = 0), npat, the table stride ml (3/5/7/8) and, per pattern, len[npat], off[npat * ml],
 * val[npat * ml], dslot[npat] (all malloc'ed: primme_amd_host_free);  1 when the matrix does not qualify: a row longer than
 * 8 entries, a 257th pattern, two entries of a row at offset 0 (one diagonal value per row is kept), an offset outside
 * int32, or offsets so far apart that a byte offset within a 512-row chunk passes 2^31;  -5 out of memory. */
#define RPD_MAXLEN 8
#define RPD_MAXPAT 256
#define RPD_SLOTS 1024                   /* open addressing, a power of two > 2 * RPD_MAXPAT */
#define RPD_CHUNK_ROWS 2048              /* what the kernel's 32-bit lane offsets are checked for: 256 lanes x 8 rows */
typedef struct { int32_t len, dslot; int32_t off[RPD_MAXLEN]; double val[RPD_MAXLEN]; } rpd_t;

static uint32_t rpd_hash(const rpd_t *p) {
   const unsigned char *b = (const unsigned char *)p;
   uint32_t h = 2166136261u;               /* FNV-1a over the (zero-padded) record */
   for (size_t i = 0; i < sizeof(rpd_t); i++) { h ^= b[i]; h *= 16777619u; }
   return h;
}

int primme_amd_csr_row_patterns_diag(int64_t m, int64_t row0, const int32_t *rp, const int32_t *ci, const void *values,
      int is_float, uint8_t **pid_out, int *npat_out, int *ml_out, int32_t **len_out, int32_t **off_out, double **val_out,
      int32_t **dslot_out) {
   *pid_out = NULL; *len_out = NULL; *off_out = NULL; *val_out = NULL; *dslot_out = NULL; *npat_out = 0; *ml_out = 0;
   if (m <= 0) return 1;
   rpd_t *pats = (rpd_t *)malloc(sizeof(rpd_t) * RPD_MAXPAT);
   int16_t *slot = (int16_t *)malloc(sizeof(int16_t) * RPD_SLOTS);
   uint8_t *pid = (uint8_t *)calloc((size_t)m + 1, 1);
   if (!pats || !slot || !pid) { free(pats); free(slot); free(pid); return -5; }
   for (int i = 0; i < RPD_SLOTS; i++) slot[i] = -1;
   int npat = 0, maxlen = 0, prev = -1, rc = 0;
   rpd_t cur;
   for (int64_t i = 0; i < m && !rc; i++) {
      const int len = rp[i + 1] - rp[i];
      if (len > RPD_MAXLEN || len < 0) { rc = 1; break; }
      memset(&cur, 0, sizeof cur);
      cur.len = len; cur.dslot = -1;
      for (int e = 0; e < len; e++) {
         const int64_t off = (int64_t)ci[rp[i] + e] - (row0 + i);
         if (off > INT32_MAX || off < INT32_MIN) { rc = 1; break; }
         cur.off[e] = (int32_t)off;
         if (off == 0) {
            if (cur.dslot >= 0) { rc = 1; break; }       /* a second diagonal entry */
            cur.dslot = e;                                 /* its value stays 0 in the key */
         } else cur.val[e] = is_float ? (double)((const float *)values)[rp[i] + e] : ((const double *)values)[rp[i] + e];
      }
      if (rc) break;
      int id = -1;
      if (prev >= 0 && !memcmp(&pats[prev], &cur, sizeof cur)) id = prev;     /* the common case: same as the row above */
      else {
         uint32_t h = rpd_hash(&cur) & (RPD_SLOTS - 1);
         while (slot[h] >= 0 && memcmp(&pats[slot[h]], &cur, sizeof cur)) h = (h + 1) & (RPD_SLOTS - 1);
         if (slot[h] >= 0) id = slot[h];
         else {
            if (npat >= RPD_MAXPAT) { rc = 1; break; }
            id = npat;
            pats[npat++] = cur;
            slot[h] = (int16_t)id;
         }
      }
      pid[i] = (uint8_t)id;
      prev = id;
      if (len > maxlen) maxlen = len;
   }
   if (!rc) {
      int64_t minoff = 0, maxoff = 0;
      for (int p = 0; p < npat; p++)
         for (int e = 0; e < pats[p].len; e++) {
            if (pats[p].off[e] < minoff) minoff = pats[p].off[e];
            if (pats[p].off[e] > maxoff) maxoff = pats[p].off[e];
         }
      if ((maxoff - minoff + RPD_CHUNK_ROWS) * (int64_t)(is_float ? 4 : 8) >= ((int64_t)1 << 31)) rc = 1;
   }
   free(slot);
   if (rc) { free(pats); free(pid); return rc; }
   const int ml = maxlen <= 3 ? 3 : maxlen <= 5 ? 5 : maxlen <= 7 ? 7 : 8;
   int32_t *tlen = (int32_t *)calloc((size_t)npat, sizeof(int32_t)), *tds = (int32_t *)calloc((size_t)npat, sizeof(int32_t));
   int32_t *toff = (int32_t *)calloc((size_t)npat * ml, sizeof(int32_t));
   double *tval = (double *)calloc((size_t)npat * ml, sizeof(double));
   if (!tlen || !tds || !toff || !tval) { free(pats); free(pid); free(tlen); free(tds); free(toff); free(tval); return -5; }
   for (int p = 0; p < npat; p++) {
      tlen[p] = pats[p].len; tds[p] = pats[p].dslot;
      for (int e = 0; e < pats[p].len; e++) { toff[(size_t)p * ml + e] = pats[p].off[e]; tval[(size_t)p * ml + e] = pats[p].val[e]; }
   }
   free(pats);
   *pid_out = pid; *npat_out = npat; *ml_out = ml; *len_out = tlen; *off_out = toff; *val_out = tval; *dslot_out = tds;
   return 0;
}

/* Sliced-ELL form of a CSR matrix, SELL-64-256 (device: hipk_sparse_sell.hip; layout: include/primme_amd_io.h).  Rows are
 * sorted by descending length inside windows of 256 consecutive rows (stable: equal lengths keep their order), the sorted
 * rows are the SLOTS, 64 consecutive slots are a SLICE, and a slice stores its entries column-major, padded to its longest
 * row.  Returns 0 and the form;  1 (nothing allocated) when the padded entries exceed max_padding * nnz or the matrix is
 * empty;  -4 when a row is longer than 65 535 entries;  -5 out of memory. */
void primme_amd_sliced_free(primme_amd_sliced *S) {
   if (!S) return;
   free(S->base); free(S->cmin); free(S->perm); free(S->len); free(S->val); free(S->idx);
   free(S);
}

int primme_amd_csr_to_sliced(int64_t m, const int32_t *rp, const int32_t *ci, const void *values, size_t elem_size,
      double max_padding, primme_amd_sliced **out) {
   *out = NULL;
   if (m <= 0 || rp[m] <= 0) return 1;
   const int64_t nnz = rp[m], nslices = (m + 63) / 64, nslots = nslices * 64;
   primme_amd_sliced *S = (primme_amd_sliced *)calloc(1, sizeof *S);
   if (!S) return -5;
   S->m = m; S->nnz = nnz; S->nslices = nslices;
   S->base = (int64_t *)calloc((size_t)nslices + 1, sizeof(int64_t));
   S->cmin = (int32_t *)calloc((size_t)nslices, sizeof(int32_t));
   S->perm = (uint8_t *)calloc((size_t)nslots, 1);
   S->len = (uint16_t *)calloc((size_t)nslots, sizeof(uint16_t));
   int32_t *start = (int32_t *)malloc(sizeof(int32_t) * 65538);
   if (!S->base || !S->cmin || !S->perm || !S->len || !start) { free(start); primme_amd_sliced_free(S); return -5; }
   /* the slots: a counting sort by length inside every window keeps equal lengths in row order */
   for (int64_t w0 = 0; w0 < m; w0 += 256) {
      const int nr = (int)(m - w0 < 256 ? m - w0 : 256);
      int maxlen = 0;
      for (int r = 0; r < nr; r++) {
         const int64_t len = (int64_t)rp[w0 + r + 1] - rp[w0 + r];
         if (len < 0 || len > 65535) { free(start); primme_amd_sliced_free(S); return -4; }
         if (len > maxlen) maxlen = (int)len;
      }
      /* start[len] = first slot of the rows of that length, longest first; rows then take their slots in row order */
      memset(start, 0, sizeof(int32_t) * ((size_t)maxlen + 2));
      for (int r = 0; r < nr; r++) start[rp[w0 + r + 1] - rp[w0 + r]]++;
      for (int len = maxlen, k = 0; len >= 0; len--) { const int c = start[len]; start[len] = k; k += c; }
      for (int r = 0; r < nr; r++) {
         const int len = rp[w0 + r + 1] - rp[w0 + r], k = start[len]++;
         S->perm[w0 + k] = (uint8_t)r; S->len[w0 + k] = (uint16_t)len;
      }
   }
   free(start);
   /* widths, bases, column spans; padded counts the entries of the slots that exist (the ragged last slice is ALLOCATED
    * 64 wide like the others, so that slot l's entry j is at base + 64 j + l everywhere) */
   int64_t padded = 0, span_max = 0;
   for (int64_t s = 0; s < nslices; s++) {
      const int ns = (int)(m - s * 64 < 64 ? m - s * 64 : 64);
      const int width = S->len[s * 64];                     /* sorted: the slice's first slot is its longest row */
      int64_t lo = INT64_MAX, hi = -1;
      for (int l = 0; l < ns; l++) {
         const int64_t row = (s * 64 / 256) * 256 + S->perm[s * 64 + l];
         for (int32_t p = rp[row]; p < rp[row + 1]; p++) { if (ci[p] < lo) lo = ci[p]; if (ci[p] > hi) hi = ci[p]; }
      }
      S->cmin[s] = hi >= lo ? (int32_t)lo : 0;
      if (hi >= lo && hi - lo > span_max) span_max = hi - lo;
      S->base[s + 1] = S->base[s] + (int64_t)width * 64;
      padded += (int64_t)width * ns;
   }
   S->padded = padded;
   if ((double)padded > max_padding * (double)nnz) { primme_amd_sliced_free(S); return 1; }
   S->idx16 = span_max < 65536;
   const size_t is = S->idx16 ? 2 : 4;
   const int64_t total = S->base[nslices];
   S->val = calloc((size_t)(total > 0 ? total : 1), elem_size);
   S->idx = calloc((size_t)(total > 0 ? total : 1), is);
   if (!S->val || !S->idx) { primme_amd_sliced_free(S); return -5; }
   if (!S->idx16) for (int64_t s = 0; s < nslices; s++) S->cmin[s] = 0;      /* 32-bit entries are the columns themselves */
   /* padding: value 0 (calloc) and the slice's first column (entry 0 against cmin), or, 32-bit, a column of the matrix */
   const int32_t anycol = ci[0];
   if (!S->idx16) for (int64_t q = 0; q < total; q++) ((int32_t *)S->idx)[q] = anycol;
   for (int64_t s = 0; s < nslices; s++) {
      const int ns = (int)(m - s * 64 < 64 ? m - s * 64 : 64);
      for (int l = 0; l < ns; l++) {
         const int64_t row = (s * 64 / 256) * 256 + S->perm[s * 64 + l];
         for (int j = 0; j < S->len[s * 64 + l]; j++) {
            const int64_t q = S->base[s] + (int64_t)j * 64 + l, p = (int64_t)rp[row] + j;
            memcpy((char *)S->val + (size_t)q * elem_size, (const char *)values + (size_t)p * elem_size, elem_size);
            if (S->idx16) ((uint16_t *)S->idx)[q] = (uint16_t)(ci[p] - S->cmin[s]);
            else ((int32_t *)S->idx)[q] = ci[p];
         }
      }
   }
   *out = S;
   return 0;
}

/* The host analysis of the row-tile kernels (device: hipk_sparse.hip, hipk_complex.hip; fields: include/primme_amd_io.h).
 * Consecutive rows are binned greedily into tiles of at most PRIMME_AMD_TILE_NNZ nonzeros and PRIMME_AMD_TILE_ROWS rows, a
 * single longer row is a tile of its own.  One pass over the rows gives the halo extent and the diagonal, one pass over every
 * tile its column window.  Returns 0 and *out, -5 out of memory. */
void primme_amd_tile_plan_free(primme_amd_tile_plan *P) {
   if (!P) return;
   free(P->tiles); free(P->info); free(P->win); free(P->diag); free(P->col16);
   free(P);
}

int primme_amd_csr_tile_plan(int64_t nrows, int64_t row0, int64_t x0, int64_t xlen, int64_t ncols_global, const int32_t *rp,
      const int32_t *ci, const void *values, size_t elem_size, int real_values, primme_amd_tile_plan **out) {
   *out = NULL;
   primme_amd_tile_plan *P = (primme_amd_tile_plan *)calloc(1, sizeof *P);
   if (!P) return -5;
   /* at most one tile per row; the records and windows carry one zero element behind the last tile */
   P->tiles = (int32_t *)calloc((size_t)nrows + 1, sizeof(int32_t));
   P->diag = calloc((size_t)(nrows > 0 ? nrows : 1), elem_size);
   if (!P->tiles || !P->diag) { primme_amd_tile_plan_free(P); return -5; }
   int64_t r = 0;
   int nt = 0;
   while (r < nrows) {
      const int64_t rs = r;
      int64_t cnt = 0;
      while (r < nrows && (r - rs) < PRIMME_AMD_TILE_ROWS) {
         const int64_t rn = rp[r + 1] - rp[r];
         if (cnt + rn > PRIMME_AMD_TILE_NNZ && r > rs) break;
         cnt += rn;
         r++;
         if (cnt > PRIMME_AMD_TILE_NNZ) break;         /* a single long row forms its own tile */
      }
      P->tiles[++nt] = (int32_t)r;
   }
   P->ntiles = nt;
   int64_t lo = 0, hi = 0;
   for (int64_t i = 0; i < nrows; i++)
      for (int32_t p = rp[i]; p < rp[i + 1]; p++) {
         const int64_t g = ci[p];
         if (g < x0 && x0 - g > lo) lo = x0 - g;
         if (g >= x0 + xlen && g - (x0 + xlen) + 1 > hi) hi = g - (x0 + xlen) + 1;
         if (g == row0 + i) memcpy((char *)P->diag + (size_t)i * elem_size, (const char *)values + (size_t)p * elem_size, elem_size);
      }
   P->halo_lo = lo; P->halo_hi = hi;
   P->info = (int32_t *)calloc(4 * ((size_t)nt + 1), sizeof(int32_t));
   P->win = (int32_t *)calloc(2 * ((size_t)nt + 1), sizeof(int32_t));
   int64_t *tmax = (int64_t *)malloc(sizeof(int64_t) * ((size_t)nt + 1));      /* last column of every tile, -1: no entry */
   if (!P->info || !P->win || !tmax) { free(tmax); primme_amd_tile_plan_free(P); return -5; }
   /* back = the farthest any tile reaches below its first row, reach = the farthest above (first row - back) */
   int64_t narrow = 0, back = 0, reach = 0;
   for (int t = 0; t < nt; t++) {
      const int32_t r0 = P->tiles[t], r1 = P->tiles[t + 1];
      int32_t *ti = P->info + 4 * (size_t)t;
      ti[0] = r0; ti[1] = r1; ti[2] = rp[r0]; ti[3] = rp[r1];
      int64_t cmin = INT64_MAX, cmax = -1;
      for (int32_t p = rp[r0]; p < rp[r1]; p++) {
         const int64_t g = ci[p];
         if (g < cmin) cmin = g;
         if (g > cmax) cmax = g;
      }
      tmax[t] = cmax;
      if (cmax >= cmin && row0 + r0 - cmin > back) back = row0 + r0 - cmin;
      /* the shifted product also reads x at the tile's own rows: they are local by construction */
      const int64_t width = cmax - cmin + 1;
      if (cmax >= cmin && cmin >= x0 && cmax < x0 + xlen && width <= PRIMME_AMD_TILE_WINDOW) {
         P->win[2 * (size_t)t] = (int32_t)cmin; P->win[2 * (size_t)t + 1] = (int32_t)width;
         if ((int)width > P->cw_max) P->cw_max = (int)width;
         if (width * 8 <= PRIMME_AMD_TILE_WINDOW) narrow++;
      }
   }
   P->windowed = (lo == 0 && hi == 0 && nt > 0 && narrow * 10 >= (int64_t)nt * 9);
   /* A second, 2-byte index stream when the pattern allows it: entry = column - (row0 + first row of the tile - c16back).
    * 10 instead of 12 bytes per nonzero out of HBM for a double matrix; the tile kernels rebuild the column from the tile
    * record they load anyway. */
   if (real_values && nt > 0) {
      for (int t = 0; t < nt; t++)
         if (rp[P->tiles[t + 1]] > rp[P->tiles[t]] && tmax[t] - (row0 + P->tiles[t] - back) > reach) reach = tmax[t] - (row0 + P->tiles[t] - back);
      if (reach <= 65535 && row0 - back > (int64_t)INT32_MIN / 2 && ncols_global < (int64_t)INT32_MAX) {
         P->col16 = (uint16_t *)calloc((size_t)rp[nrows] + 1, sizeof(uint16_t));      /* +1: clamped loads of an empty tile */
         if (!P->col16) { free(tmax); primme_amd_tile_plan_free(P); return -5; }
         P->c16back = back;
         for (int t = 0; t < nt; t++)
            for (int32_t p = rp[P->tiles[t]]; p < rp[P->tiles[t + 1]]; p++)
               P->col16[p] = (uint16_t)(ci[p] - (row0 + P->tiles[t] - back));
      }
   }
   free(tmax);
   *out = P;
   return 0;
}

/* The levels of the geometric multigrid preconditioner (primme_amd_multigrid_precond).  Level 0 is the
 * caller's grid with weights 1.  From a level to the next every dimension of 3 or more points is halved (n / 2: coarse point j
 * sits on fine point 2 j + 1) and its weight, the factor of its 1-D Laplacian in the level operator, divided by 4; shorter
 * dimensions are kept.  The last level is the first without a dimension of 3 or more points, or with at most
 * PRIMME_AMD_MG_COARSE_POINTS points, or the PRIMME_AMD_MG_MAXLEVELS-th.  n and w hold PRIMME_AMD_MG_MAXLEVELS rows; the rows
 * behind *nlevels are left alone.  Returns 0, -1 for a dimension below 1 or more than INT32_MAX points. */
int primme_amd_mg_plan(const int dims[3], int *nlevels, int n[][3], double w[][3]) {
   if (!dims || !nlevels || !n || !w) return -1;
   int64_t pts = 1;
   for (int d = 0; d < 3; d++) {
      if (dims[d] < 1) return -1;
      pts *= dims[d];
      if (pts > INT32_MAX) return -1;
      n[0][d] = dims[d]; w[0][d] = 1.0;
   }
   int l = 0;
   while (l + 1 < PRIMME_AMD_MG_MAXLEVELS && pts > PRIMME_AMD_MG_COARSE_POINTS &&
          (n[l][0] >= 3 || n[l][1] >= 3 || n[l][2] >= 3)) {
      pts = 1;
      for (int d = 0; d < 3; d++) {
         const int c = n[l][d] >= 3;
         n[l + 1][d] = c ? n[l][d] / 2 : n[l][d];
         w[l + 1][d] = c ? w[l][d] / 4.0 : w[l][d];
         pts *= n[l + 1][d];
      }
      l++;
   }
   *nlevels = l + 1;
   return 0;
}

/* ---- hierarchy of the aggregation algebraic multigrid preconditioner (primme_amd_io.h) ----------- */
static void amg_level_free(primme_amd_amg_level *L) {
   free(L->rowptr); free(L->colind); free(L->values); free(L->dinv); free(L->agg); free(L->aggptr); free(L->aggrows);
   memset(L, 0, sizeof(*L));
}
void primme_amd_amg_plan_free(primme_amd_amg_plan *plan) {
   if (!plan) return;
   for (int l = 0; l < PRIMME_AMD_AMG_MAXLEVELS; l++) {
      primme_amd_amg_transfer *X = &plan->transfer[l];
      amg_level_free(&plan->level[l]);
      free(X->prowptr); free(X->pcolind); free(X->pvalues); free(X->rrowptr); free(X->rcolind); free(X->rvalues);
   }
   free(plan);
}
static int amg_i32_cmp(const void *a, const void *b) {
   const int32_t x = *(const int32_t *)a, y = *(const int32_t *)b;
   return x < y ? -1 : x > y;
}

/* dg = diag(M_l); dinv and rho of the level.  -1: a row without a diagonal entry or with m_ii <= 0, -5: out of memory */
int pa_amg_level_finish(primme_amd_amg_level *L, double *dg) {
   L->dinv = (double *)malloc(sizeof(double) * (size_t)L->n);
   if (!L->dinv) return -5;
   double rho = 0.0;
   for (int64_t i = 0; i < L->n; i++) {
      double d = 0.0, s = 0.0;
      int found = 0;
      for (int32_t q = L->rowptr[i]; q < L->rowptr[i + 1]; q++) {
         if (L->colind[q] == i) { d += L->values[q]; found = 1; }
         s += fabs(L->values[q]);
      }
      if (!found || !(d > 0.0)) return -1;
      dg[i] = d; L->dinv[i] = 1.0 / d;
      if (s / d > rho) rho = s / d;
   }
   L->rho = rho;
   return 0;
}

/* the three passes; agg[n] receives the aggregate of every row, returns the number of aggregates.  tmp: n int32 */
int64_t pa_amg_aggregate(const primme_amd_amg_level *L, const double *dg, double theta, int32_t *agg, int32_t *tmp) {
   const int64_t n = L->n;
   const int32_t *rp = L->rowptr, *ci = L->colind;
   const double *va = L->values;
   int32_t nc = 0;
#define AMG_STRONG(i, q) (ci[q] != (i) && fabs(va[q]) >= theta * sqrt(dg[i] * dg[ci[q]]))
   for (int64_t i = 0; i < n; i++) agg[i] = tmp[i] = -1;
   for (int64_t i = 0; i < n; i++) {                       /* pass 1 */
      if (agg[i] >= 0) continue;
      int ok = 1;
      for (int32_t q = rp[i]; q < rp[i + 1] && ok; q++)
         if (AMG_STRONG(i, q) && agg[ci[q]] >= 0) ok = 0;
      if (!ok) continue;
      agg[i] = nc;
      for (int32_t q = rp[i]; q < rp[i + 1]; q++)
         if (AMG_STRONG(i, q)) agg[ci[q]] = nc;
      nc++;
   }
   for (int64_t i = 0; i < n; i++) {                       /* pass 2: agg holds the pass-1 aggregates until the loop is over */
      if (agg[i] >= 0) continue;
      int32_t best = -1;
      double bv = -1.0;
      for (int32_t q = rp[i]; q < rp[i + 1]; q++) {
         if (!AMG_STRONG(i, q) || agg[ci[q]] < 0) continue;
         const double v = fabs(va[q]);
         const int32_t a = agg[ci[q]];
         if (v > bv || (v == bv && a < best)) { bv = v; best = a; }
      }
      tmp[i] = best;
   }
   for (int64_t i = 0; i < n; i++)
      if (agg[i] < 0) agg[i] = tmp[i];
   for (int64_t i = 0; i < n; i++) {                       /* pass 3 */
      if (agg[i] >= 0) continue;
      agg[i] = nc;
      for (int32_t q = rp[i]; q < rp[i + 1]; q++)
         if (AMG_STRONG(i, q) && agg[ci[q]] < 0) agg[ci[q]] = nc;
      nc++;
   }
#undef AMG_STRONG
   return nc;
}

/* level 0 of a plan in L (zeroed): M_0 = A + shift I in double, the shift on the first diagonal entry of a row; dinv, rho and
 * dg = diag(M_0).  -1: an index out of range, a row without a diagonal entry or m_ii <= 0; -5: out of memory */
int pa_amg_level0(int64_t n, const int32_t *rowptr, const int32_t *colind, const void *values, size_t elem_size, double shift,
      primme_amd_amg_level *L, double *dg) {
   const int64_t nnz = rowptr[n];
   int rc = 0;
   L->n = n; L->nnz = nnz;
   L->rowptr = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n + 1));
   L->colind = (int32_t *)malloc(sizeof(int32_t) * (size_t)(nnz > 0 ? nnz : 1));
   L->values = (double *)malloc(sizeof(double) * (size_t)(nnz > 0 ? nnz : 1));
   if (!L->rowptr || !L->colind || !L->values) return -5;
   memcpy(L->rowptr, rowptr, sizeof(int32_t) * (size_t)(n + 1));
   memcpy(L->colind, colind, sizeof(int32_t) * (size_t)nnz);
   for (int64_t q = 0; q < nnz; q++) L->values[q] = elem_size == 8 ? ((const double *)values)[q] : (double)((const float *)values)[q];
   for (int64_t i = 0; i < n && !rc; i++) {          /* + shift on the (first) diagonal entry of the row */
      int32_t q = rowptr[i];
      while (q < rowptr[i + 1] && (colind[q] < 0 || colind[q] >= n || colind[q] != i)) {
         if (colind[q] < 0 || colind[q] >= n) rc = -1;
         q++;
      }
      for (int32_t r = q; r < rowptr[i + 1]; r++)
         if (colind[r] < 0 || colind[r] >= n) rc = -1;
      if (q < rowptr[i + 1]) L->values[q] += shift; else rc = -1;
   }
   return rc ? rc : pa_amg_level_finish(L, dg);
}

/* the aggregates of level L (pa_amg_aggregate) and their inverse map: sets nc, agg, aggptr and aggrows.  1: the aggregation
 * would keep more than 0.8 n rows and is discarded, L as it was; -5: out of memory.  tmp: n int32 */
int pa_amg_level_aggregate(primme_amd_amg_level *L, const double *dg, double theta, int32_t *tmp) {
   int32_t *agg = (int32_t *)malloc(sizeof(int32_t) * (size_t)L->n);
   if (!agg) return -5;
   const int64_t nc = pa_amg_aggregate(L, dg, theta, agg, tmp);
   if ((double)nc > 0.8 * (double)L->n) { free(agg); return 1; }
   L->agg = agg; L->nc = nc;
   L->aggptr = (int32_t *)calloc((size_t)(nc + 1), sizeof(int32_t));
   L->aggrows = (int32_t *)malloc(sizeof(int32_t) * (size_t)L->n);
   if (!L->aggptr || !L->aggrows) return -5;
   for (int64_t i = 0; i < L->n; i++) L->aggptr[agg[i] + 1]++;
   for (int64_t j = 0; j < nc; j++) L->aggptr[j + 1] += L->aggptr[j];
   for (int64_t j = 0; j < nc; j++) tmp[j] = L->aggptr[j];
   for (int64_t i = 0; i < L->n; i++) L->aggrows[tmp[agg[i]]++] = (int32_t)i;
   return 0;
}

/* C = P' F P for the aggregates of F (F->nc, agg, aggptr, aggrows are set): row I adds the rows of aggregate I in ascending
 * order, every row's entries in their order; columns sorted, one entry per position; then entry (J, I) takes the bits of
 * (I, J), I < J, so that C is exactly symmetric when its pattern is */
static int amg_galerkin(const primme_amd_amg_level *F, primme_amd_amg_level *Cl) {
   const int64_t nc = F->nc;
   Cl->n = nc;
   Cl->rowptr = (int32_t *)malloc(sizeof(int32_t) * (size_t)(nc + 1));
   Cl->colind = (int32_t *)malloc(sizeof(int32_t) * (size_t)(F->nnz > 0 ? F->nnz : 1));
   Cl->values = (double *)malloc(sizeof(double) * (size_t)(F->nnz > 0 ? F->nnz : 1));
   int32_t *mark = (int32_t *)malloc(sizeof(int32_t) * (size_t)nc), *list = (int32_t *)malloc(sizeof(int32_t) * (size_t)nc);
   double *acc = (double *)malloc(sizeof(double) * (size_t)nc);
   if (!Cl->rowptr || !Cl->colind || !Cl->values || !mark || !list || !acc) { free(mark); free(list); free(acc); return -5; }
   for (int64_t J = 0; J < nc; J++) mark[J] = -1;
   int32_t nnz = 0;
   Cl->rowptr[0] = 0;
   for (int64_t I = 0; I < nc; I++) {
      int32_t cnt = 0;
      for (int32_t p = F->aggptr[I]; p < F->aggptr[I + 1]; p++) {
         const int32_t i = F->aggrows[p];
         for (int32_t q = F->rowptr[i]; q < F->rowptr[i + 1]; q++) {
            const int32_t J = F->agg[F->colind[q]];
            if (mark[J] != (int32_t)I) { mark[J] = (int32_t)I; acc[J] = F->values[q]; list[cnt++] = J; }
            else acc[J] += F->values[q];
         }
      }
      qsort(list, (size_t)cnt, sizeof(int32_t), amg_i32_cmp);
      for (int32_t k = 0; k < cnt; k++) { Cl->colind[nnz] = list[k]; Cl->values[nnz] = acc[list[k]]; nnz++; }
      Cl->rowptr[I + 1] = nnz;
   }
   free(mark); free(list); free(acc);
   Cl->nnz = nnz;
   for (int64_t I = 0; I < nc; I++)
      for (int32_t q = Cl->rowptr[I]; q < Cl->rowptr[I + 1]; q++) {
         const int32_t J = Cl->colind[q];
         if (J <= I) continue;
         int32_t lo = Cl->rowptr[J], hi = Cl->rowptr[J + 1];
         while (lo < hi) {
            const int32_t mid = lo + (hi - lo) / 2;
            if (Cl->colind[mid] < (int32_t)I) lo = mid + 1; else hi = mid;
         }
         if (lo < Cl->rowptr[J + 1] && Cl->colind[lo] == (int32_t)I) Cl->values[lo] = Cl->values[q];
      }
   return 0;
}

/* P = (I - (omega / rho) D^-1 M) T for the aggregates of F (nc, agg set; dinv and rho too) and its transpose R.  Row i of P:
 * the sums s_J of m_iq over the entries q with agg[col q] = J, in the row's order, then p_iJ = [J = agg[i]] - (omega / rho)
 * dinv_i s_J; columns sorted, one entry per position, an entry that cancels to zero stays.  R by a counting sort over the
 * columns of P: rows of R have ascending column indices and the bits of P. */
int pa_amg_prolongation(const primme_amd_amg_level *F, double omega, primme_amd_amg_transfer *X) {
   const int64_t n = F->n, nc = F->nc;
   const double w = omega / F->rho;
   int rc = 0;
   X->prowptr = (int32_t *)malloc(sizeof(int32_t) * (size_t)(n + 1));
   X->pcolind = (int32_t *)malloc(sizeof(int32_t) * (size_t)(F->nnz + n));      /* a row of P has at most the row of M and agg[i] */
   X->pvalues = (double *)malloc(sizeof(double) * (size_t)(F->nnz + n));
   X->rrowptr = (int32_t *)calloc((size_t)(nc + 1), sizeof(int32_t));
   int32_t *mark = (int32_t *)malloc(sizeof(int32_t) * (size_t)nc), *list = (int32_t *)malloc(sizeof(int32_t) * (size_t)nc);
   double *acc = (double *)malloc(sizeof(double) * (size_t)nc);
   if (!X->prowptr || !X->pcolind || !X->pvalues || !X->rrowptr || !mark || !list || !acc) rc = -5;
   int64_t nnz = 0;
   if (!rc) {
      for (int64_t J = 0; J < nc; J++) mark[J] = -1;
      X->prowptr[0] = 0;
   }
   for (int64_t i = 0; i < n && !rc; i++) {
      const int32_t own = F->agg[i];
      int32_t cnt = 0;
      mark[own] = (int32_t)i; acc[own] = 0.0; list[cnt++] = own;
      for (int32_t q = F->rowptr[i]; q < F->rowptr[i + 1]; q++) {
         const int32_t J = F->agg[F->colind[q]];
         if (mark[J] != (int32_t)i) { mark[J] = (int32_t)i; acc[J] = F->values[q]; list[cnt++] = J; }
         else acc[J] += F->values[q];
      }
      if (nnz + cnt > INT32_MAX) { rc = -4; break; }
      qsort(list, (size_t)cnt, sizeof(int32_t), amg_i32_cmp);
      const double c = w * F->dinv[i];
      for (int32_t k = 0; k < cnt; k++) {
         const int32_t J = list[k];
         X->pcolind[nnz] = J;
         X->pvalues[nnz] = (J == own ? 1.0 : 0.0) - c * acc[J];
         X->rrowptr[J + 1]++;
         nnz++;
      }
      X->prowptr[i + 1] = (int32_t)nnz;
   }
   free(mark); free(list); free(acc);
   if (rc) return rc;
   X->pnnz = nnz;
   X->rcolind = (int32_t *)malloc(sizeof(int32_t) * (size_t)(nnz > 0 ? nnz : 1));
   X->rvalues = (double *)malloc(sizeof(double) * (size_t)(nnz > 0 ? nnz : 1));
   int32_t *cur = (int32_t *)malloc(sizeof(int32_t) * (size_t)nc);
   if (!X->rcolind || !X->rvalues || !cur) { free(cur); return -5; }
   for (int64_t J = 0; J < nc; J++) { X->rrowptr[J + 1] += X->rrowptr[J]; cur[J] = X->rrowptr[J]; }
   for (int64_t i = 0; i < n; i++)
      for (int32_t p = X->prowptr[i]; p < X->prowptr[i + 1]; p++) {
         const int32_t at = cur[X->pcolind[p]]++;
         X->rcolind[at] = (int32_t)i; X->rvalues[at] = X->pvalues[p];
      }
   free(cur);
   return 0;
}

/* C = R F P for the transfer matrices X of F (R = P').  Row I of the upper triangle: over the entries (i, r) of row I of R
 * in their order, the entries (k, m) of row i of F in theirs and the entries (J, p) of row k of P with J >= I in theirs,
 * c_IJ += (r m) p; columns sorted, one entry per position.  Entry (J, I) then takes the bits of (I, J): C is exactly
 * symmetric.  -4 when C would have more than INT32_MAX entries. */
int pa_amg_galerkin_general(const primme_amd_amg_level *F, const primme_amd_amg_transfer *X, primme_amd_amg_level *Cl) {
   const int64_t nc = F->nc;
   int rc = 0;
   int64_t cap = F->nnz > 16 ? F->nnz : 16, unnz = 0;
   int32_t *urp = (int32_t *)malloc(sizeof(int32_t) * (size_t)(nc + 1)), *uci = (int32_t *)malloc(sizeof(int32_t) * (size_t)cap);
   double *uva = (double *)malloc(sizeof(double) * (size_t)cap);
   int32_t *mark = (int32_t *)malloc(sizeof(int32_t) * (size_t)nc), *list = (int32_t *)malloc(sizeof(int32_t) * (size_t)nc);
   int32_t *cnt = (int32_t *)calloc((size_t)(nc + 1), sizeof(int32_t));
   double *acc = (double *)malloc(sizeof(double) * (size_t)nc);
   if (!urp || !uci || !uva || !mark || !list || !cnt || !acc) rc = -5;
   if (!rc) {
      for (int64_t J = 0; J < nc; J++) mark[J] = -1;
      urp[0] = 0;
   }
   int64_t total = 0;
   for (int64_t I = 0; I < nc && !rc; I++) {
      int32_t len = 0;
      for (int32_t a = X->rrowptr[I]; a < X->rrowptr[I + 1]; a++) {
         const int32_t i = X->rcolind[a];
         const double r = X->rvalues[a];
         for (int32_t q = F->rowptr[i]; q < F->rowptr[i + 1]; q++) {
            const int32_t k = F->colind[q];
            const double rm = r * F->values[q];
            for (int32_t t = X->prowptr[k]; t < X->prowptr[k + 1]; t++) {
               const int32_t J = X->pcolind[t];
               if (J < (int32_t)I) continue;
               if (mark[J] != (int32_t)I) { mark[J] = (int32_t)I; acc[J] = rm * X->pvalues[t]; list[len++] = J; }
               else acc[J] += rm * X->pvalues[t];
            }
         }
      }
      if (unnz + len > cap) {
         while (unnz + len > cap) cap *= 2;
         int32_t *nci = (int32_t *)realloc(uci, sizeof(int32_t) * (size_t)cap);
         if (nci) uci = nci;
         double *nva = (double *)realloc(uva, sizeof(double) * (size_t)cap);
         if (nva) uva = nva;
         if (!nci || !nva) { rc = -5; break; }
      }
      qsort(list, (size_t)len, sizeof(int32_t), amg_i32_cmp);
      for (int32_t k = 0; k < len; k++) {
         const int32_t J = list[k];
         uci[unnz] = J; uva[unnz] = acc[J]; unnz++;
         cnt[I]++;
         if (J != (int32_t)I) cnt[J]++;
      }
      total += 2 * (int64_t)len - (len > 0 && list[0] == (int32_t)I ? 1 : 0);
      if (unnz > INT32_MAX || total > INT32_MAX) { rc = -4; break; }
      urp[I + 1] = (int32_t)unnz;
   }
   free(mark); free(list); free(acc);
   if (!rc) {
      Cl->n = nc; Cl->nnz = total;
      Cl->rowptr = (int32_t *)malloc(sizeof(int32_t) * (size_t)(nc + 1));
      Cl->colind = (int32_t *)malloc(sizeof(int32_t) * (size_t)(total > 0 ? total : 1));
      Cl->values = (double *)malloc(sizeof(double) * (size_t)(total > 0 ? total : 1));
      if (!Cl->rowptr || !Cl->colind || !Cl->values) rc = -5;
   }
   if (!rc) {
      Cl->rowptr[0] = 0;
      for (int64_t I = 0; I < nc; I++) { Cl->rowptr[I + 1] = Cl->rowptr[I] + cnt[I]; cnt[I] = Cl->rowptr[I]; }
      /* rows ascending: when row I is reached, its entries left of the diagonal are in place */
      for (int64_t I = 0; I < nc; I++)
         for (int32_t u = urp[I]; u < urp[I + 1]; u++) {
            const int32_t J = uci[u];
            Cl->colind[cnt[I]] = J; Cl->values[cnt[I]] = uva[u]; cnt[I]++;
            if (J != (int32_t)I) { Cl->colind[cnt[J]] = (int32_t)I; Cl->values[cnt[J]] = uva[u]; cnt[J]++; }
         }
   }
   free(urp); free(uci); free(uva); free(cnt);
   return rc;
}

static int amg_plan_build(int64_t n, const int32_t *rowptr, const int32_t *colind, const void *values, size_t elem_size,
      double shift, double theta, double omega, primme_amd_amg_plan **plan) {
   if (!plan) return -1;
   *plan = NULL;
   if (n < 1 || !rowptr || !colind || !values || (elem_size != 8 && elem_size != 4) || !(shift >= 0.0) || !(theta >= 0.0 && theta < 1.0)) return -1;
   if (n > INT32_MAX) return -4;
   primme_amd_amg_plan *P = (primme_amd_amg_plan *)calloc(1, sizeof(*P));
   double *dg = (double *)malloc(sizeof(double) * (size_t)n);
   int32_t *tmp = (int32_t *)malloc(sizeof(int32_t) * (size_t)n);
   int rc = (P && dg && tmp) ? 0 : -5;
   if (!rc) {
      P->shift = shift; P->theta = theta; P->omega = omega;
      rc = pa_amg_level0(n, rowptr, colind, values, elem_size, shift, &P->level[0], dg);
   }
   int l = 0;
   while (!rc) {
      primme_amd_amg_level *L = &P->level[l];
      if (L->n <= PRIMME_AMD_AMG_DENSE_ROWS || l + 1 >= PRIMME_AMD_AMG_MAXLEVELS) break;
      rc = pa_amg_level_aggregate(L, dg, theta, tmp);
      if (rc) { rc = rc > 0 ? 0 : rc; break; }                           /* 1: stalled, this level is the last */
      if (omega == 0.0) rc = amg_galerkin(L, &P->level[l + 1]);
      else {
         rc = pa_amg_prolongation(L, omega, &P->transfer[l]);
         if (!rc) rc = pa_amg_galerkin_general(L, &P->transfer[l], &P->level[l + 1]);
      }
      if (!rc) rc = pa_amg_level_finish(&P->level[l + 1], dg);
      l++;
   }
   free(dg); free(tmp);
   if (rc) { primme_amd_amg_plan_free(P); return rc; }
   P->nlevels = l + 1;
   *plan = P;
   return 0;
}

int primme_amd_amg_plan_create(int64_t n, const int32_t *rowptr, const int32_t *colind, const void *values, size_t elem_size,
      double shift, double theta, primme_amd_amg_plan **plan) {
   return amg_plan_build(n, rowptr, colind, values, elem_size, shift, theta, 0.0, plan);
}

int primme_amd_amg_plan_create_smoothed(int64_t n, const int32_t *rowptr, const int32_t *colind, const void *values, size_t elem_size,
      double shift, double theta, double omega, primme_amd_amg_plan **plan) {
   if (!plan) return -1;
   *plan = NULL;
   if (!(omega > 0.0 && omega < 2.0)) return -1;
   return amg_plan_build(n, rowptr, colind, values, elem_size, shift, theta, omega, plan);
}

int primme_amd_amg_coarse_inverse(const primme_amd_amg_plan *plan, double *G) {
   if (!plan || !G || plan->nlevels < 1) return -1;
   const primme_amd_amg_level *L = &plan->level[plan->nlevels - 1];
   const int n = (int)L->n;
   if (L->n > PRIMME_AMD_AMG_DENSE_ROWS) return -1;
   double *C = (double *)calloc((size_t)n * n, sizeof(double));
   if (!C) return -5;
   for (int i = 0; i < n; i++)
      for (int32_t q = L->rowptr[i]; q < L->rowptr[i + 1]; q++) C[(size_t)i * n + L->colind[q]] += L->values[q];
   /* M = C C' (lower triangle of C, row-major) */
   for (int j = 0; j < n; j++) {
      double d = C[(size_t)j * n + j];
      for (int k = 0; k < j; k++) d -= C[(size_t)j * n + k] * C[(size_t)j * n + k];
      if (!(d > 0.0)) { free(C); return -1; }
      d = sqrt(d);
      C[(size_t)j * n + j] = d;
      for (int i = j + 1; i < n; i++) {
         double s = C[(size_t)i * n + j];
         for (int k = 0; k < j; k++) s -= C[(size_t)i * n + k] * C[(size_t)j * n + k];
         C[(size_t)i * n + j] = s / d;
      }
   }
   /* column c of the inverse: C z = e_c, C' g = z */
   for (int c = 0; c < n; c++) {
      double *g = G + (size_t)c * n;
      for (int i = 0; i < n; i++) {
         double s = i == c ? 1.0 : 0.0;
         for (int k = c; k < i; k++) s -= C[(size_t)i * n + k] * g[k];
         g[i] = i < c ? 0.0 : s / C[(size_t)i * n + i];
      }
      for (int i = n - 1; i >= 0; i--) {
         double s = g[i];
         for (int k = i + 1; k < n; k++) s -= C[(size_t)k * n + i] * g[k];
         g[i] = s / C[(size_t)i * n + i];
      }
   }
   free(C);
   for (int i = 0; i < n; i++)
      for (int j = 0; j < i; j++) {
         const double s = 0.5 * (G[(size_t)i * n + j] + G[(size_t)j * n + i]);
         G[(size_t)i * n + j] = G[(size_t)j * n + i] = s;
      }
   return 0;
}
