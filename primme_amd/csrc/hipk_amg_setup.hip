/* hipk_amg_setup.hip — the row-parallel stages of the smoothed-aggregation set-up on the device (gfx950): what
 * primme_amd_amg_hierarchy_create runs per level when it is asked for the device set-up.
 *
 *   hipk_amg_build_prolongation   P = (I - w D^-1 M) T for the aggregate map of T, w = omega / rho
 *   hipk_amg_csr_transpose        R = P' with ascending columns and the bits of P
 *   hipk_amg_galerkin             C = R (M P): B = M P, the upper triangle U of R B, C = strict(U)' + U
 *   hipk_amg_level_finish         dinv = 1 / diag, diag, rho = max_i sum_j |m_ij| / m_ii and the flag of a bad diagonal
 *
 * Every matrix is CSR with int32 indices, double values, ascending columns in a row and one entry per position.
 *
 * Owner per output row.  The rows are dealt as hipk_amg_csr_apply deals them: a wave takes 64 consecutive rows per trip, lane l
 * row base + l.  A row whose DRIVING row (the row of M for P and B, of R for U, of the matrix itself for the sort and the finish)
 * has at most 64 entries is built by its lane; a longer one afterwards by the whole wave, one such row at a time, found with a
 * ballot: trip loop and long-row loop are wave-uniform, all 64 lanes reach every ballot and shuffle.
 *
 * A sparse row is built by SELECTION, without a hash table and without scratch: the owner sweeps the contributions of the row for
 * the smallest column above the last one it emitted and for that column's value, emits both, and repeats until a sweep finds
 * nothing.  Columns come out ascending and once each; the sweep visits the contributions in the order of the driving row, so
 * every sum has one order.  The loop ends because the emitted column grows strictly and is below the column count; its bound is
 * written out.  The operand rows are sorted, so a sweep leaves a row at its first column above the last emitted one; the
 * products keep a cursor per entry of the driving matrix (an int32 array of its size, the stage's only scratch beside B and U), so
 * that a row of B is walked once per output row and not once per emitted column, which matters on the small coarse levels with
 * hundreds of entries per row (the table of stages per level).
 * Two phases: the symbolic pass runs the same selection and stores the row's count, an exclusive scan (three plain launches:
 * chunk sums, the scan of the chunk sums by one workgroup, the chunks again) turns counts into row pointers, the numeric pass
 * fills.  The totals are read back between the phases: the arrays of a product are allocated at their exact size, and a total
 * beyond the entry limit (INT32_MAX) or a failed allocation ends the stage with 1, nothing kept: the caller falls back.
 *
 * Deterministic: no floating-point atomics.  Integer atomics count the entries of a column (the transpose), claim a slot in the
 * column's segment (the claim order is erased by the sort of the segment by row index, which are distinct), raise the flag and
 * take the maximum of the non-negative ratios through their bit patterns; none of the results depends on the order.
 * No workgroup waits for another.  P must be the host's bits: 1 - c s is a product and a difference with a rounding each
 * (contraction is switched off for that expression), s summed in the row's order; a long row gives every lane one emitted column and
 * lets all lanes walk the row together, each adding what belongs to its column.
 * Accesses: the operands are read by element through indices (rows of P through colind of M, agg through colind); the scan
 * moves 16 bytes per lane and access.  The entry points check sizes and pointers and TRUST the indices.  No reference counterpart. */
#include "hipk_internal.h"
#include "primme_amd_io.h"

#define SETUP_LANE_LEN 64
#define SETUP_NONE 0x7fffffff
#define SCAN_PER 8                                /* consecutive counts per lane */
#define SCAN_CHUNK (HIPK_BLOCK * SCAN_PER)

/* the entry limit a caller passes: negative or beyond int32 reads as INT32_MAX */
static int64_t setup_limit(int64_t max_entries) { return max_entries < 0 || max_entries > INT32_MAX ? INT32_MAX : max_entries; }

/* ---- the dealer ------------------------------------------------------------------------------------------------------- */
template <class Op>
__global__ void __launch_bounds__(HIPK_BLOCK) setup_rows_kernel(int64_t nrows, Op op) {
   const int lane = threadIdx.x & (HIPK_WAVE - 1);
   const int64_t nwaves = (int64_t)gridDim.x * (HIPK_BLOCK / HIPK_WAVE);
   const int64_t wave = (int64_t)blockIdx.x * (HIPK_BLOCK / HIPK_WAVE) + (threadIdx.x / HIPK_WAVE);
   for (int64_t base = wave * HIPK_WAVE; base < nrows; base += nwaves * HIPK_WAVE) {
      const int64_t j = base + lane;
      int32_t p0 = 0, p1 = 0;
      if (j < nrows) { p0 = op.rowptr[j]; p1 = op.rowptr[j + 1]; }
      const bool is_long = p1 - p0 > SETUP_LANE_LEN;
      if (j < nrows && !is_long) op.lane_row(j, p0, p1);
      unsigned long long mask = __ballot(is_long);
      while (mask) {
         const int src = __ffsll((long long)mask) - 1;
         mask &= mask - 1;
         op.wave_row(base + src, __shfl(p0, src), __shfl(p1, src), lane);
      }
   }
}
static __device__ __forceinline__ int32_t wave_min(int32_t v) {
   for (int o = HIPK_WAVE / 2; o > 0; o >>= 1) { const int32_t u = __shfl_xor(v, o); v = u < v ? u : v; }
   return v;
}
static __device__ __forceinline__ double wave_sum(double v) {
   for (int o = HIPK_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
   return v;
}

/* ---- P = (I - w D^-1 M) T ---------------------------------------------------------------------------------------------- */
/* delta - c s with a rounding after the product and one after the difference, as the host forms it */
static __device__ __forceinline__ double prolong_value(double delta, double c, double s) {
#pragma clang fp contract(off)
   const double t = c * s;
   return delta - t;
}
template <bool NUMERIC> struct prolong_op {
   const int32_t *rowptr, *colind, *agg;
   const double *values, *dinv;
   double w;
   int32_t *count;                                /* symbolic: the row's entries */
   const int32_t *prowptr;                        /* numeric */
   int32_t *pcolind;
   double *pvalues;
   __device__ void lane_row(int64_t i, int32_t p0, int32_t p1) const {
      const int32_t own = agg[i], len = p1 - p0;
      const double c = w * dinv[i];
      const int32_t o = NUMERIC ? prowptr[i] : 0;
      int32_t prev = -1, cnt = 0;
      for (int32_t it = 0; it <= len; it++) {                /* at most len + 1 columns */
         int32_t best = own > prev ? own : SETUP_NONE;
         for (int32_t q = p0; q < p1; q++) {
            const int32_t J = agg[colind[q]];
            if (J > prev && J < best) best = J;
         }
         if (best == SETUP_NONE) break;
         if (NUMERIC) {
            double s = 0.0;
            for (int32_t q = p0; q < p1; q++)
               if (agg[colind[q]] == best) s += values[q];
            pcolind[o + cnt] = best;
            pvalues[o + cnt] = prolong_value(best == own ? 1.0 : 0.0, c, s);
         }
         cnt++; prev = best;
      }
      if (!NUMERIC) count[i] = cnt;
   }
   __device__ void wave_row(int64_t i, int32_t q0, int32_t q1, int lane) const {
      const int32_t own = agg[i], len = q1 - q0;
      const double c = w * dinv[i];
      const int32_t o = NUMERIC ? prowptr[i] : 0;
      int32_t prev = -1, cnt = 0, mine = -1, filled = 0;
      bool done = false;
      for (int32_t it = 0; it < len + 2 && !done; it++) {    /* len + 1 columns at most, and the sweep that finds none */
         int32_t best = (lane == 0 && own > prev) ? own : SETUP_NONE;
         for (int32_t q = q0 + lane; q < q1; q += HIPK_WAVE) {
            const int32_t J = agg[colind[q]];
            if (J > prev && J < best) best = J;
         }
         best = wave_min(best);
         if (best == SETUP_NONE) done = true;
         else {
            if (lane == filled) mine = best;
            filled++; cnt++; prev = best;
         }
         if (filled == HIPK_WAVE || (done && filled > 0)) {
            if (NUMERIC) {                                   /* lane l sums the column it holds, all lanes walk the row together */
               double s = 0.0;
               for (int32_t q = q0; q < q1; q++)
                  if (agg[colind[q]] == mine) s += values[q];
               if (lane < filled) {
                  pcolind[o + cnt - filled + lane] = mine;
                  pvalues[o + cnt - filled + lane] = prolong_value(mine == own ? 1.0 : 0.0, c, s);
               }
            }
            filled = 0; mine = -1;
         }
      }
      if (!NUMERIC && lane == 0) count[i] = cnt;
   }
};

/* ---- C = A B, or its upper triangle -------------------------------------------------------------------------------------- */
template <bool NUMERIC, bool TRIU> struct product_op {
   const int32_t *rowptr, *colind;                /* A */
   const double *values;
   const int32_t *brp, *bci;                      /* B */
   const double *bva;
   int64_t ncols;                                 /* of B */
   int32_t *count;
   const int32_t *crp;
   int32_t *cci;
   double *cva;
   int32_t *cursor;                               /* one per entry of A: how far the row of B it names has been consumed */
   /* the contribution of entry q of the driving row to the smallest column above prev: best and sum are updated.  The rows
      of B are sorted and prev only grows, so the cursor of q only advances: over a whole output row the walks add up to the
      length of the row of B (finite from its row pointers), not to one walk per emitted column.  cursor[q] belongs to the
      lane that owns q, in every sweep. */
   __device__ __forceinline__ void sweep(int32_t q, int32_t prev, int32_t &best, double &sum) const {
      const int32_t t1 = brp[colind[q] + 1];
      int32_t t = cursor[q];
      while (t < t1 && bci[t] <= prev) t++;
      cursor[q] = t;
      if (t >= t1) return;
      const int32_t J = bci[t];
      if (J < best) { best = J; sum = values[q] * bva[t]; }
      else if (J == best) sum = fma(values[q], bva[t], sum);
   }
   __device__ void lane_row(int64_t i, int32_t p0, int32_t p1) const {
      const int32_t o = NUMERIC ? crp[i] : 0;
      int32_t prev = TRIU ? (int32_t)i - 1 : -1, cnt = 0;
      for (int32_t q = p0; q < p1; q++) cursor[q] = brp[colind[q]];
      for (int64_t it = 0; it <= ncols; it++) {              /* the emitted column grows strictly and is below ncols */
         int32_t best = SETUP_NONE;
         double sum = 0.0;
         for (int32_t q = p0; q < p1; q++) sweep(q, prev, best, sum);
         if (best == SETUP_NONE) break;
         if (NUMERIC) { cci[o + cnt] = best; cva[o + cnt] = sum; }
         cnt++; prev = best;
      }
      if (!NUMERIC) count[i] = cnt;
   }
   __device__ void wave_row(int64_t i, int32_t q0, int32_t q1, int lane) const {
      const int32_t o = NUMERIC ? crp[i] : 0;
      int32_t prev = TRIU ? (int32_t)i - 1 : -1, cnt = 0;
      for (int32_t q = q0 + lane; q < q1; q += HIPK_WAVE) cursor[q] = brp[colind[q]];
      for (int64_t it = 0; it <= ncols; it++) {
         int32_t mine = SETUP_NONE;
         double sum = 0.0;
         for (int32_t q = q0 + lane; q < q1; q += HIPK_WAVE) sweep(q, prev, mine, sum);
         const int32_t best = wave_min(mine);
         if (best == SETUP_NONE) break;                      /* wave-uniform */
         if (NUMERIC) {
            const double s = wave_sum(mine == best ? sum : 0.0);
            if (lane == 0) { cci[o + cnt] = best; cva[o + cnt] = s; }
         }
         cnt++; prev = best;
      }
      if (!NUMERIC && lane == 0) count[i] = cnt;
   }
};

/* ---- the transpose: counts, claimed slots, and the sort of a segment by row index -------------------------------------------- */
template <bool CLAIM>
__global__ void __launch_bounds__(HIPK_BLOCK) transpose_scatter_kernel(int64_t nrows, int strict, const int32_t *__restrict__ rowptr,
      const int32_t *__restrict__ colind, int32_t *cursor, int32_t *wrow, int32_t *wpos) {
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < nrows; i += stride) {
      const int32_t p1 = rowptr[i + 1];
      for (int32_t p = rowptr[i]; p < p1; p++) {
         const int32_t J = colind[p];
         if (strict && J == (int32_t)i) continue;
         const int32_t at = atomicAdd(&cursor[J], 1);
         if (CLAIM) { wrow[at] = (int32_t)i; wpos[at] = p; }
      }
   }
}
struct sort_op {
   const int32_t *rowptr;                         /* of the transpose */
   const int32_t *wrow, *wpos;
   const double *values;                          /* of the source */
   int32_t *tci;
   double *tva;
   __device__ void lane_row(int64_t j, int32_t p0, int32_t p1) const {
      for (int32_t e = p0; e < p1; e++) {
         const int32_t key = wrow[e];
         int32_t rank = 0;
         for (int32_t f = p0; f < p1; f++) rank += wrow[f] < key;
         tci[p0 + rank] = key; tva[p0 + rank] = values[wpos[e]];
      }
   }
   __device__ void wave_row(int64_t j, int32_t q0, int32_t q1, int lane) const {
      for (int32_t e = q0 + lane; e < q1; e += HIPK_WAVE) {
         const int32_t key = wrow[e];
         int32_t rank = 0;
         for (int32_t f = q0; f < q1; f++) rank += wrow[f] < key;
         tci[q0 + rank] = key; tva[q0 + rank] = values[wpos[e]];
      }
   }
};

/* C = L + U row by row, L the strict lower triangle (the transpose of the strict upper one) */
__global__ void __launch_bounds__(HIPK_BLOCK) merge_rowptr_kernel(int64_t n1, const int32_t *__restrict__ lrp, const int32_t *__restrict__ urp, int32_t *crp) {
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < n1; i += stride) crp[i] = lrp[i] + urp[i];
}
struct merge_op {
   const int32_t *rowptr;                         /* of C */
   const int32_t *lrp, *lci, *urp, *uci;
   const double *lva, *uva;
   int32_t *cci;
   double *cva;
   __device__ void lane_row(int64_t i, int32_t p0, int32_t p1) const {
      const int32_t l0 = lrp[i], nl = lrp[i + 1] - l0, u0 = urp[i];
      for (int32_t e = 0; e < p1 - p0; e++) {
         cci[p0 + e] = e < nl ? lci[l0 + e] : uci[u0 + e - nl];
         cva[p0 + e] = e < nl ? lva[l0 + e] : uva[u0 + e - nl];
      }
   }
   __device__ void wave_row(int64_t i, int32_t q0, int32_t q1, int lane) const {
      const int32_t l0 = lrp[i], nl = lrp[i + 1] - l0, u0 = urp[i];
      for (int32_t e = lane; e < q1 - q0; e += HIPK_WAVE) {
         cci[q0 + e] = e < nl ? lci[l0 + e] : uci[u0 + e - nl];
         cva[q0 + e] = e < nl ? lva[l0 + e] : uva[u0 + e - nl];
      }
   }
};

/* ---- dinv, diag, rho and the flag ---------------------------------------------------------------------------------------- */
struct finish_op {
   const int32_t *rowptr, *colind;
   const double *values;
   double *dinv, *diag;
   unsigned long long *rho_bits;
   int *flag;
   __device__ __forceinline__ void store(int64_t i, double d, double s, bool found) const {
      dinv[i] = 1.0 / d;
      if (diag) diag[i] = d;
      if (!found || !(d > 0.0)) { atomicOr(flag, 1); return; }
      const double ratio = s / d;
      if (ratio >= 0.0) atomicMax(rho_bits, (unsigned long long)__double_as_longlong(ratio));   /* order of the bits = order of the values */
   }
   __device__ void lane_row(int64_t i, int32_t p0, int32_t p1) const {
      double d = 0.0, s = 0.0;
      bool found = false;
      for (int32_t q = p0; q < p1; q++) {
         if (colind[q] == (int32_t)i) { d += values[q]; found = true; }
         s += fabs(values[q]);
      }
      store(i, d, s, found);
   }
   /* rho is compared with the host's to a few ulp, and a sum of hundreds of terms in another order is farther off than that:
      a long row is summed in the row's order too, by all lanes alike (every load is one address for the wave) */
   __device__ void wave_row(int64_t i, int32_t q0, int32_t q1, int lane) const {
      double d = 0.0, s = 0.0;
      bool found = false;
      for (int32_t q = q0; q < q1; q++) {
         if (colind[q] == (int32_t)i) { d += values[q]; found = true; }
         s += fabs(values[q]);
      }
      if (lane == 0) store(i, d, s, found);
   }
};

/* ---- exclusive scan of int32 counts, in place allowed: out[i] = sum of in[0 .. i), out[n] = the total ------------------------ */
struct alignas(16) scan_i4 { int32_t v[4]; };
static __device__ __forceinline__ void scan_load(const int32_t *in, int64_t n, int64_t first, bool wide, int32_t v[SCAN_PER]) {
   if (wide && first + SCAN_PER <= n) {
#pragma unroll
      for (int e = 0; e < SCAN_PER; e += 4) {
         const scan_i4 x = *(const scan_i4 *)(in + first + e);
         v[e] = x.v[0]; v[e + 1] = x.v[1]; v[e + 2] = x.v[2]; v[e + 3] = x.v[3];
      }
   } else {
#pragma unroll
      for (int e = 0; e < SCAN_PER; e++) v[e] = first + e < n ? in[first + e] : 0;
   }
}
/* exclusive scan of one value per thread over the workgroup; *total: the sum */
static __device__ __forceinline__ int64_t block_exclusive(int64_t v, int64_t *sh, int64_t *total) {
   const int t = threadIdx.x;
   sh[t] = v;
   __syncthreads();
   for (int o = 1; o < HIPK_BLOCK; o <<= 1) {
      const int64_t u = t >= o ? sh[t - o] : 0;
      __syncthreads();
      sh[t] += u;
      __syncthreads();
   }
   const int64_t incl = sh[t];
   *total = sh[HIPK_BLOCK - 1];
   __syncthreads();
   return incl - v;
}
__global__ void __launch_bounds__(HIPK_BLOCK) scan_sums_kernel(int64_t n, int wide, const int32_t *in, int64_t *chunk) {
   __shared__ int64_t sh[HIPK_BLOCK];
   int32_t v[SCAN_PER];
   scan_load(in, n, (int64_t)blockIdx.x * SCAN_CHUNK + (int64_t)threadIdx.x * SCAN_PER, wide != 0, v);
   int64_t s = 0, total;
#pragma unroll
   for (int e = 0; e < SCAN_PER; e++) s += v[e];
   (void)block_exclusive(s, sh, &total);
   if (threadIdx.x == 0) chunk[blockIdx.x] = total;
}
/* one workgroup: chunk[b] becomes the sum of the chunks before b, chunk[nchunks] the total */
__global__ void __launch_bounds__(HIPK_BLOCK) scan_chunks_kernel(int64_t nchunks, int64_t *chunk) {
   __shared__ int64_t sh[HIPK_BLOCK];
   int64_t carry = 0;
   for (int64_t b0 = 0; b0 < nchunks; b0 += HIPK_BLOCK) {    /* wave-uniform: every thread takes every trip */
      const int64_t b = b0 + threadIdx.x;
      const int64_t v = b < nchunks ? chunk[b] : 0;
      int64_t total;
      const int64_t ex = block_exclusive(v, sh, &total);
      if (b < nchunks) chunk[b] = carry + ex;
      carry += total;
   }
   if (threadIdx.x == 0) chunk[nchunks] = carry;
}
__global__ void __launch_bounds__(HIPK_BLOCK) scan_apply_kernel(int64_t n, int wide, const int32_t *in, const int64_t *chunk, int32_t *out) {
   __shared__ int64_t sh[HIPK_BLOCK];
   int32_t v[SCAN_PER];
   const int64_t first = (int64_t)blockIdx.x * SCAN_CHUNK + (int64_t)threadIdx.x * SCAN_PER;
   scan_load(in, n, first, wide != 0, v);
   int64_t s = 0, total;
#pragma unroll
   for (int e = 0; e < SCAN_PER; e++) s += v[e];
   int64_t run = chunk[blockIdx.x] + block_exclusive(s, sh, &total);      /* every load of the workgroup is behind its barriers */
   if (wide && first + SCAN_PER <= n) {
#pragma unroll
      for (int e = 0; e < SCAN_PER; e += 4) {
         scan_i4 x;
#pragma unroll
         for (int k = 0; k < 4; k++) { x.v[k] = (int32_t)run; run += v[e + k]; }
         *(scan_i4 *)(out + first + e) = x;
      }
   } else {
#pragma unroll
      for (int e = 0; e < SCAN_PER; e++)
         if (first + e < n) { out[first + e] = (int32_t)run; run += v[e]; }
   }
   if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[n] = (int32_t)chunk[gridDim.x];
}

/* ---- host side --------------------------------------------------------------------------------------------------------- */
static int setup_num_cu(void) {
   static int num_cu = 0;                      /* launch geometry only: read the device once */
   if (num_cu == 0) {
      int dev = 0, n = 0;
      if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) num_cu = n;
      else num_cu = 256;
   }
   return num_cu;
}
/* workgroups for `items` items, `per` of them per workgroup and trip, at most eight workgroups per compute unit */
static unsigned setup_grid(int64_t items, int64_t per) {
   const int64_t cap = (int64_t)setup_num_cu() * 8;
   int64_t gx = (items + per - 1) / per;
   if (gx > cap) gx = cap;
   return (unsigned)(gx < 1 ? 1 : gx);
}
template <class Op> static void setup_rows(hipStream_t st, int64_t nrows, const Op &op) {
   hipLaunchKernelGGL((setup_rows_kernel<Op>), dim3(setup_grid(nrows, HIPK_BLOCK)), dim3(HIPK_BLOCK), 0, st, nrows, op);
}
/* a device array of `count` elements; 1: no memory (the error is cleared), 0: fine */
template <typename T> static int setup_alloc(T **p, int64_t count) {
   *p = NULL;
   if (hipMalloc((void **)p, sizeof(T) * (size_t)(count > 0 ? count : 1)) != hipSuccess) { (void)hipGetLastError(); *p = NULL; return 1; }
   return 0;
}
static void setup_free(void *p) { if (p) (void)hipFree(p); }
/* counts[0 .. n) -> offsets[0 .. n], in place allowed; *total on the host, the stream synchronised.  1: no memory */
static int setup_scan(hipStream_t st, int64_t n, const int32_t *counts, int32_t *offsets, int64_t *total) {
   const int64_t nchunks = (n + SCAN_CHUNK - 1) / SCAN_CHUNK;
   int64_t *chunk = NULL;
   if (setup_alloc(&chunk, nchunks + 1)) return 1;
   const int wide = (((uintptr_t)counts | (uintptr_t)offsets) & 15) == 0;
   hipLaunchKernelGGL(scan_sums_kernel, dim3((unsigned)nchunks), dim3(HIPK_BLOCK), 0, st, n, wide, counts, chunk);
   hipLaunchKernelGGL(scan_chunks_kernel, dim3(1), dim3(HIPK_BLOCK), 0, st, nchunks, chunk);
   hipLaunchKernelGGL(scan_apply_kernel, dim3((unsigned)nchunks), dim3(HIPK_BLOCK), 0, st, n, wide, counts, (const int64_t *)chunk, offsets);
   int rc = 0;
   if (hipMemcpyAsync(total, chunk + nchunks, sizeof(int64_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess ||
       hipGetLastError() != hipSuccess) rc = -1;
   setup_free(chunk);
   return rc;
}

extern "C" int hipk_amg_build_prolongation(void *hip_stream, int64_t n, int64_t nc, const int32_t *rowptr, const int32_t *colind,
      const double *values, const double *dinv, const int32_t *agg, double w, int64_t max_entries, int32_t **prowptr, int32_t **pcolind, double **pvalues, int64_t *pnnz) {
   if (n < 1 || nc < 1 || nc > n || n > INT32_MAX - 1 || !rowptr || !colind || !values || !dinv || !agg || !prowptr || !pcolind || !pvalues || !pnnz) return -1;
   hipStream_t st = (hipStream_t)hip_stream;
   int32_t *prp = NULL, *pci = NULL;
   double *pva = NULL;
   int64_t total = 0;
   *prowptr = NULL; *pcolind = NULL; *pvalues = NULL; *pnnz = 0;
   if (setup_alloc(&prp, n + 1)) return 1;
   prolong_op<false> sym = {rowptr, colind, agg, values, dinv, w, prp, NULL, NULL, NULL};
   setup_rows(st, n, sym);
   int rc = setup_scan(st, n, prp, prp, &total);
   if (!rc && total > setup_limit(max_entries)) rc = 1;
   if (!rc) rc = setup_alloc(&pci, total) | setup_alloc(&pva, total);
   if (!rc) {
      prolong_op<true> num = {rowptr, colind, agg, values, dinv, w, NULL, prp, pci, pva};
      setup_rows(st, n, num);
      if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) rc = -1;
   }
   if (rc) { setup_free(prp); setup_free(pci); setup_free(pva); return rc; }
   *prowptr = prp; *pcolind = pci; *pvalues = pva; *pnnz = total;
   return 0;
}

/* T = A' (strict: without the diagonal entries of A) for an nrows x ncols matrix A; *tnnz its entries */
static int setup_transpose(hipStream_t st, int64_t limit, int64_t nrows, int64_t ncols, int strict, const int32_t *rowptr, const int32_t *colind, const double *values,
      int64_t nnz, int32_t **trowptr, int32_t **tcolind, double **tvalues, int64_t *tnnz) {
   int32_t *trp = NULL, *tci = NULL, *cursor = NULL, *wrow = NULL, *wpos = NULL;
   double *tva = NULL;
   int64_t total = 0;
   *trowptr = NULL; *tcolind = NULL; *tvalues = NULL; *tnnz = 0;
   int rc = setup_alloc(&trp, ncols + 1) | setup_alloc(&cursor, ncols);
   if (!rc && hipMemsetAsync(trp, 0, sizeof(int32_t) * (size_t)(ncols + 1), st) != hipSuccess) rc = -1;
   if (!rc) {
      hipLaunchKernelGGL((transpose_scatter_kernel<false>), dim3(setup_grid(nrows, HIPK_BLOCK)), dim3(HIPK_BLOCK), 0, st, nrows, strict, rowptr, colind, trp,
            (int32_t *)NULL, (int32_t *)NULL);
      rc = setup_scan(st, ncols, trp, trp, &total);
   }
   if (!rc && (total > nnz || total > limit)) rc = total > nnz ? -1 : 1;
   if (!rc) rc = setup_alloc(&tci, total) | setup_alloc(&tva, total) | setup_alloc(&wrow, total) | setup_alloc(&wpos, total);
   if (!rc && hipMemcpyAsync(cursor, trp, sizeof(int32_t) * (size_t)ncols, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = -1;
   if (!rc) {
      hipLaunchKernelGGL((transpose_scatter_kernel<true>), dim3(setup_grid(nrows, HIPK_BLOCK)), dim3(HIPK_BLOCK), 0, st, nrows, strict, rowptr, colind, cursor, wrow, wpos);
      sort_op so = {trp, wrow, wpos, values, tci, tva};
      setup_rows(st, ncols, so);
      if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) rc = -1;
   }
   setup_free(cursor); setup_free(wrow); setup_free(wpos);
   if (rc) { setup_free(trp); setup_free(tci); setup_free(tva); return rc; }
   *trowptr = trp; *tcolind = tci; *tvalues = tva; *tnnz = total;
   return 0;
}

extern "C" int hipk_amg_csr_transpose(void *hip_stream, int64_t nrows, int64_t ncols, int64_t nnz, const int32_t *rowptr, const int32_t *colind,
      const double *values, int64_t max_entries, int32_t **trowptr, int32_t **tcolind, double **tvalues) {
   if (nrows < 1 || ncols < 1 || nrows > INT32_MAX - 1 || ncols > INT32_MAX - 1 || nnz < 0 || nnz > INT32_MAX || !rowptr || !colind || !values ||
       !trowptr || !tcolind || !tvalues) return -1;
   int64_t tnnz = 0;
   const int rc = setup_transpose((hipStream_t)hip_stream, setup_limit(max_entries), nrows, ncols, 0, rowptr, colind, values, nnz, trowptr, tcolind, tvalues, &tnnz);
   if (!rc && tnnz != nnz) { setup_free(*trowptr); setup_free(*tcolind); setup_free(*tvalues); *trowptr = NULL; *tcolind = NULL; *tvalues = NULL; return -1; }
   return rc;
}

/* C = A B (triu: the entries (i, j >= i) only), A nrows x nmid, B nmid x ncols; symbolic pass, scan, numeric pass */
template <bool TRIU>
static int setup_product(hipStream_t st, int64_t limit, int64_t nrows, int64_t ncols, const int32_t *arp, const int32_t *aci, const double *ava,
      const int32_t *brp, const int32_t *bci, const double *bva, int32_t **crowptr, int32_t **ccolind, double **cvalues, int64_t *cnnz) {
   int32_t *crp = NULL, *cci = NULL;
   double *cva = NULL;
   int64_t total = 0;
   *crowptr = NULL; *ccolind = NULL; *cvalues = NULL; *cnnz = 0;
   int32_t annz = 0, *cursor = NULL;             /* the entries of A: a cursor each */
   if (hipMemcpyAsync(&annz, arp + nrows, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess || annz < 0) return -1;
   if (setup_alloc(&crp, nrows + 1)) return 1;
   if (setup_alloc(&cursor, annz)) { setup_free(crp); return 1; }
   product_op<false, TRIU> sym = {arp, aci, ava, brp, bci, bva, ncols, crp, NULL, NULL, NULL, cursor};
   setup_rows(st, nrows, sym);
   int rc = setup_scan(st, nrows, crp, crp, &total);
   if (!rc && total > limit) rc = 1;
   if (!rc) rc = setup_alloc(&cci, total) | setup_alloc(&cva, total);
   if (!rc) {
      product_op<true, TRIU> num = {arp, aci, ava, brp, bci, bva, ncols, NULL, crp, cci, cva, cursor};
      setup_rows(st, nrows, num);
      if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) rc = -1;
   }
   setup_free(cursor);
   if (rc) { setup_free(crp); setup_free(cci); setup_free(cva); return rc; }
   *crowptr = crp; *ccolind = cci; *cvalues = cva; *cnnz = total;
   return 0;
}

extern "C" int hipk_amg_galerkin(void *hip_stream, int64_t n, int64_t nc, const int32_t *rowptr, const int32_t *colind, const double *values,
      const int32_t *prowptr, const int32_t *pcolind, const double *pvalues, const int32_t *rrowptr, const int32_t *rcolind, const double *rvalues,
      int64_t max_entries, int32_t **crowptr, int32_t **ccolind, double **cvalues, int64_t *cnnz) {
   if (n < 1 || nc < 1 || nc > n || n > INT32_MAX - 1 || !rowptr || !colind || !values || !prowptr || !pcolind || !pvalues || !rrowptr || !rcolind ||
       !rvalues || !crowptr || !ccolind || !cvalues || !cnnz) return -1;
   hipStream_t st = (hipStream_t)hip_stream;
   const int64_t limit = setup_limit(max_entries);
   int32_t *brp = NULL, *bci = NULL, *urp = NULL, *uci = NULL, *lrp = NULL, *lci = NULL, *crp = NULL, *cci = NULL;
   double *bva = NULL, *uva = NULL, *lva = NULL, *cva = NULL;
   int64_t bnnz = 0, unnz = 0, lnnz = 0;
   *crowptr = NULL; *ccolind = NULL; *cvalues = NULL; *cnnz = 0;
   int rc = setup_product<false>(st, limit, n, nc, rowptr, colind, values, prowptr, pcolind, pvalues, &brp, &bci, &bva, &bnnz);
   if (!rc) rc = setup_product<true>(st, limit, nc, nc, rrowptr, rcolind, rvalues, brp, bci, bva, &urp, &uci, &uva, &unnz);
   setup_free(brp); setup_free(bci); setup_free(bva);
   if (!rc) rc = setup_transpose(st, limit, nc, nc, 1, urp, uci, uva, unnz, &lrp, &lci, &lva, &lnnz);
   if (!rc && lnnz + unnz > limit) rc = 1;
   if (!rc) rc = setup_alloc(&crp, nc + 1) | setup_alloc(&cci, lnnz + unnz) | setup_alloc(&cva, lnnz + unnz);
   if (!rc) {
      hipLaunchKernelGGL(merge_rowptr_kernel, dim3(setup_grid(nc + 1, HIPK_BLOCK)), dim3(HIPK_BLOCK), 0, st, nc + 1, (const int32_t *)lrp, (const int32_t *)urp, crp);
      merge_op mo = {crp, lrp, lci, urp, uci, lva, uva, cci, cva};
      setup_rows(st, nc, mo);
      if (hipStreamSynchronize(st) != hipSuccess || hipGetLastError() != hipSuccess) rc = -1;
   }
   setup_free(urp); setup_free(uci); setup_free(uva); setup_free(lrp); setup_free(lci); setup_free(lva);
   if (rc) { setup_free(crp); setup_free(cci); setup_free(cva); return rc; }
   *crowptr = crp; *ccolind = cci; *cvalues = cva; *cnnz = lnnz + unnz;
   return 0;
}

extern "C" int hipk_amg_level_finish(void *hip_stream, int64_t n, const int32_t *rowptr, const int32_t *colind, const double *values,
      double *dinv, double *diag, double *rho, int *flag) {
   if (n < 1 || n > INT32_MAX - 1 || !rowptr || !colind || !values || !dinv || !rho || !flag) return -1;
   hipStream_t st = (hipStream_t)hip_stream;
   unsigned long long *res = NULL;                /* [0]: the bits of rho, [1]: the flag */
   if (setup_alloc(&res, 2)) return 1;
   int rc = 0;
   if (hipMemsetAsync(res, 0, 2 * sizeof(*res), st) != hipSuccess) rc = -1;
   unsigned long long host[2] = {0, 0};
   if (!rc) {
      finish_op fo = {rowptr, colind, values, dinv, diag, res, (int *)(res + 1)};
      setup_rows(st, n, fo);
      if (hipMemcpyAsync(host, res, sizeof(host), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess ||
          hipGetLastError() != hipSuccess) rc = -1;
   }
   setup_free(res);
   if (rc) return rc;
   memcpy(rho, &host[0], sizeof(double));
   *flag = (int)(host[1] & 0xffffffffull) != 0;
   return 0;
}

extern "C" void hipk_amg_setup_free(void *device_array) { setup_free(device_array); }
