/* hipk_panels.hip — tall-skinny panel kernels of the Davidson inner loop (gfx950): the TN inner products and the
 * Gram-Schmidt updates.  The fused Ritz / residual / restart family is in hipk_ritz.hip, the column utilities and
 * the QMR vector passes are in hipk_vec.hip; what the three share is in hipk_panel_dev.h.
 *
 * All of these are HBM-bound streaming kernels: every basis column is read once
 * per launch with unit-stride wave accesses (64 lanes x 8 B = 512 B per
 * instruction, NC independent loads in flight per lane), reductions go
 * lane -> wave (DPP shuffles) -> workgroup (LDS) -> per-block partial, and a tiny
 * second launch adds the partials in a fixed order so results are bit-reproducible
 * run to run and identical on every rank.
 *
 * What each kernel replaces in the reference is listed in
 * include/primme_amd_kernels.h.
 */
#include "hipk_panel_dev.h"

/* finalize with an output leading dimension: out[(o % nrows) + (o / nrows)*ldout] */
__global__ void __launch_bounds__(HIPK_BLOCK)
finalize_ld_kernel(const double *__restrict__ partials, int nblocks, int nout, int nrows,
      int ldout, double *__restrict__ out, double *__restrict__ out_host, hipk_fin_flag fin) {
   __shared__ double sm[HIPK_BLOCK / HIPK_WAVE];
   const int o = blockIdx.x;
   double s = 0.0;
   for (int b = threadIdx.x; b < nblocks; b += HIPK_BLOCK) s += partials[(size_t)b * nout + o];
   s = hipk_wave_sum(s);
   if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
   __syncthreads();
   if (threadIdx.x == 0) {
      const double v = (sm[0] + sm[1]) + (sm[2] + sm[3]);
      const size_t at = (o % nrows) + (size_t)(o / nrows) * ldout;
      out[at] = v;
      if (out_host) out_host[at] = v;
      hipk_publish_flag(fin, gridDim.x);
   }
}

/* ============================ TN: inner products ============================== */
template <typename T, int NC, int NX, int VW>
__global__ void __launch_bounds__(HIPK_BLOCK)
dots_kernel(SegArgs segs, const T *__restrict__ X, int64_t ldX, int nx, int64_t m,
      double *__restrict__ partials) {
   typedef lanevec<T, VW> LV;
   const int j0 = blockIdx.y * NC;             /* first basis column of this chunk */
   const int c0 = blockIdx.z * NX;             /* first right-hand column          */
   const int ncv = min(NC, segs.total - j0);
   const int nxv = min(NX, nx - c0);
   const T *cp[NC];
#pragma unroll
   for (int jj = 0; jj < NC; jj++) cp[jj] = seg_col<T>(segs, jj < ncv ? j0 + jj : j0);
   const T *xp = X + (size_t)c0 * (size_t)ldX;

   double acc[NC][NX];
#pragma unroll
   for (int jj = 0; jj < NC; jj++)
#pragma unroll
      for (int c = 0; c < NX; c++) acc[jj][c] = 0.0;

   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   const int64_t mg = m / VW;                   /* full lane groups */
   for (int64_t g = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; g < mg; g += stride) {
      LV xv[NX], a[NC];
#pragma unroll
      for (int c = 0; c < NX; c++)
         if (c < nxv) xv[c] = ((const LV *)(xp + (size_t)c * ldX))[g];
#pragma unroll
      for (int jj = 0; jj < NC; jj++)
         if (jj < ncv) a[jj] = ldstream<T, VW, 16>(cp[jj], g);
#pragma unroll
      for (int jj = 0; jj < NC; jj++)
         if (jj < ncv) {
#pragma unroll
            for (int c = 0; c < NX; c++)
               if (c < nxv) {
#pragma unroll
                  for (int r = 0; r < VW; r++) acc[jj][c] = fma((double)a[jj].e[r], (double)xv[c].e[r], acc[jj][c]);
               }
         }
   }
   if (VW > 1 && blockIdx.x == 0 && threadIdx.x < (unsigned)(m - mg * VW)) {   /* ragged tail rows */
      const int64_t i = mg * VW + threadIdx.x;
#pragma unroll
      for (int jj = 0; jj < NC; jj++)
         if (jj < ncv) {
#pragma unroll
            for (int c = 0; c < NX; c++)
               if (c < nxv) acc[jj][c] = fma((double)cp[jj][i], (double)xp[i + (size_t)c * ldX], acc[jj][c]);
         }
   }

   __shared__ double sm[HIPK_BLOCK / HIPK_WAVE][NC * NX];
   const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
   for (int jj = 0; jj < NC; jj++)
#pragma unroll
      for (int c = 0; c < NX; c++) {
         double v = hipk_wave_sum(acc[jj][c]);
         if (lane == 0) sm[wv][jj * NX + c] = v;
      }
   __syncthreads();
   if (threadIdx.x < NC * NX) {
      const int jj = threadIdx.x / NX, c = threadIdx.x % NX;
      if (jj < ncv && c < nxv) {
         double v = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
         partials[(size_t)blockIdx.x * ((size_t)segs.total * nx) + (size_t)(j0 + jj) +
                  (size_t)(c0 + c) * segs.total] = v;
      }
   }
}

/* Several right-hand columns (block methods): one WAVE per chunk of NC basis columns, all waves of
 * a workgroup walk the SAME rows, so the NX right-hand columns are fetched from HBM once per
 * workgroup (the other waves hit the CU's L1) instead of once per column chunk.  Each wave reduces
 * its own NC x NX block of the result; no cross-wave reduction is needed. */
template <typename T, int NC, int NX, int VW, int WAVES>
__global__ void __launch_bounds__(64 * WAVES)
dots_wide_kernel(SegArgs segs, const T *__restrict__ X, int64_t ldX, int nx, int64_t m,
      double *__restrict__ partials) {
   typedef lanevec<T, VW> LV;
   const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
   const int j0 = (blockIdx.y * WAVES + wv) * NC;
   const int c0 = blockIdx.z * NX;
   const int ncv = min(NC, segs.total - j0);     /* <= 0: this wave has no columns (still walks along) */
   const int nxv = min(NX, nx - c0);
   const T *cp[NC];
#pragma unroll
   for (int jj = 0; jj < NC; jj++) cp[jj] = seg_col<T>(segs, (jj < ncv) ? j0 + jj : 0);
   const T *xp = X + (size_t)c0 * (size_t)ldX;
   double acc[NC][NX];
#pragma unroll
   for (int jj = 0; jj < NC; jj++)
#pragma unroll
      for (int c = 0; c < NX; c++) acc[jj][c] = 0.0;
   const int64_t stride = (int64_t)gridDim.x * 64;
   const int64_t mg = m / VW;
   if (ncv > 0) {
      for (int64_t g = (int64_t)blockIdx.x * 64 + lane; g < mg; g += stride) {
         LV xv[NX], a[NC];
#pragma unroll
         for (int c = 0; c < NX; c++)
            if (c < nxv) xv[c] = ((const LV *)(xp + (size_t)c * ldX))[g];
#pragma unroll
         for (int jj = 0; jj < NC; jj++)
            if (jj < ncv) a[jj] = ldstream<T, VW, 16>(cp[jj], g);
#pragma unroll
         for (int jj = 0; jj < NC; jj++)
            if (jj < ncv) {
#pragma unroll
               for (int c = 0; c < NX; c++)
                  if (c < nxv) {
#pragma unroll
                     for (int r = 0; r < VW; r++) acc[jj][c] = fma((double)a[jj].e[r], (double)xv[c].e[r], acc[jj][c]);
                  }
            }
      }
      if (VW > 1 && blockIdx.x == 0 && lane < (int)(m - mg * VW)) {
         const int64_t i = mg * VW + lane;
#pragma unroll
         for (int jj = 0; jj < NC; jj++)
            if (jj < ncv) {
#pragma unroll
               for (int c = 0; c < NX; c++)
                  if (c < nxv) acc[jj][c] = fma((double)cp[jj][i], (double)xp[i + (size_t)c * ldX], acc[jj][c]);
            }
      }
#pragma unroll
      for (int jj = 0; jj < NC; jj++)
#pragma unroll
         for (int c = 0; c < NX; c++) {
            const double v = hipk_wave_sum(acc[jj][c]);
            if (lane == 0 && jj < ncv && c < nxv)
               partials[(size_t)blockIdx.x * ((size_t)segs.total * nx) + (size_t)(j0 + jj) + (size_t)(c0 + c) * segs.total] = v;
         }
   }
}

/* Blocks of right-hand columns on the matrix cores: G = [Q V]' X with v_mfma_f64_16x16x4_f64
 * (reference: Num_gemm_ddh / Num_compute_gramm, cublas_wrapper.c:479-499, :898-987; the b >= 4 TN
 * panels of Bortho_block_gen and update_projection).  A workgroup stages MF_ROWS rows of up to
 * 16*NT basis columns and of the (<= 16) right-hand columns in LDS with fully coalesced 16-byte
 * loads — each wave fetches whole columns, 1 KB per instruction — and then feeds the MFMA from
 * LDS: for a 16x16x4 step the k index is a ROW of the panels, lane l supplies
 * A[i = l & 15][k = l >> 4] = V(row, column i) and B[k = l >> 4][j = l & 15] = X(row, column j).
 * The column stride in LDS is MF_ROWS + 2 doubles (= 2 mod 32), which makes the 32 lanes of a
 * ds_read_b64 group hit 32 distinct bank pairs.  Wave w takes the k-steps of rows [32 w, 32 w + 32)
 * of the staged tile for every (basis tile, X) pair; the 4-double accumulators (C/D layout of the
 * f64 form: column = lane & 15, row = (lane >> 4) + 4 reg) stay in registers for the whole row
 * range of the workgroup and the four waves' partial tiles are added in a fixed order at the end.
 * An NT x 16-column tile of accumulators costs 8 NT VGPRs per lane where the FMA form
 * (dots_wide_kernel<8, 8>) holds 64 accumulators in 128. */
#define MF_ROWS 128
#define MF_LDS_STRIDE (MF_ROWS + 2)
typedef double mf_acc __attribute__((ext_vector_type(4)));

template <typename T, int NT>
__global__ void __launch_bounds__(HIPK_BLOCK)
dots_mfma_kernel(SegArgs segs, const T *__restrict__ X, int64_t ldX, int nx, int64_t m,
      double *__restrict__ partials) {
   typedef lanevec<T, 2> LV;
   extern __shared__ double mf_lds[];            /* [(16*NT + 16) columns][MF_LDS_STRIDE] */
   const int lane = threadIdx.x & 63;
   const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
   const int j0 = blockIdx.y * 16 * NT;          /* first basis column of this workgroup */
   const int ncv = min(16 * NT, segs.total - j0);
   const int c0 = blockIdx.z * 16;               /* first right-hand column */
   const int nxv = min(16, nx - c0);
   double *sV = mf_lds, *sX = mf_lds + (size_t)16 * NT * MF_LDS_STRIDE;
   mf_acc acc[NT];
#pragma unroll
   for (int t = 0; t < NT; t++) acc[t] = (mf_acc){0.0, 0.0, 0.0, 0.0};
   const int ci = lane & 15, kg = lane >> 4;

   const int64_t ntile = (m + MF_ROWS - 1) / MF_ROWS;
   for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
      const int64_t r0 = tile * MF_ROWS;
      const bool full = r0 + MF_ROWS <= m;
      /* stage: wave w fetches columns w, w + 4, ... (2 rows per lane, 1 KB per column); every load is
       * issued before the first LDS store, absent columns read a valid one and are zeroed afterwards */
      constexpr int NCW = (16 * NT + 16) / 4;
      LV tv[NCW];
      if (full) {
#pragma unroll
         for (int q = 0; q < NCW; q++) {
            const int c = wv + 4 * q;
            const bool isx = c >= 16 * NT;
            const int cc = isx ? c - 16 * NT : c;
            const T *col = isx ? X + (size_t)(c0 + (cc < nxv ? cc : 0)) * ldX : seg_col<T>(segs, j0 + (cc < ncv ? cc : 0));
            tv[q] = ((const LV *)(col + r0))[lane];
         }
      } else {
#pragma unroll
         for (int q = 0; q < NCW; q++) {
            const int c = wv + 4 * q;
            const bool isx = c >= 16 * NT;
            const int cc = isx ? c - 16 * NT : c;
            const T *col = isx ? X + (size_t)(c0 + (cc < nxv ? cc : 0)) * ldX : seg_col<T>(segs, j0 + (cc < ncv ? cc : 0));
            const int64_t i = r0 + 2 * lane;
            const T e0 = col[i < m ? i : m - 1], e1 = col[i + 1 < m ? i + 1 : m - 1];
            tv[q].e[0] = i < m ? e0 : (T)0;
            tv[q].e[1] = i + 1 < m ? e1 : (T)0;
         }
      }
#pragma unroll
      for (int q = 0; q < NCW; q++) {
         const int c = wv + 4 * q;
         const bool isx = c >= 16 * NT;
         const int cc = isx ? c - 16 * NT : c;
         const bool have = isx ? (cc < nxv) : (cc < ncv);
         double *dstc = mf_lds + (size_t)c * MF_LDS_STRIDE + 2 * lane;
         dstc[0] = have ? (double)tv[q].e[0] : 0.0;
         dstc[1] = have ? (double)tv[q].e[1] : 0.0;
      }
      __syncthreads();
      /* 8 k-steps of 4 rows for this wave */
#pragma unroll
      for (int st = 0; st < MF_ROWS / 16; st++) {
         const int row = wv * (MF_ROWS / 4) + 4 * st + kg;
         const double b = sX[(size_t)ci * MF_LDS_STRIDE + row];
#pragma unroll
         for (int t = 0; t < NT; t++) {
            const double a = sV[(size_t)(16 * t + ci) * MF_LDS_STRIDE + row];
            acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[t], 0, 0, 0);
         }
      }
      __syncthreads();
   }
   /* add the four waves' tiles in a fixed order: red[wave][tile][reg][lane] in the staging buffer */
   double *red = mf_lds;
#pragma unroll
   for (int t = 0; t < NT; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) red[(((size_t)wv * NT + t) * 4 + r) * 64 + lane] = acc[t][r];
   __syncthreads();
   if (wv == 0) {
      const size_t nout = (size_t)segs.total * nx;
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
         for (int r = 0; r < 4; r++) {
            const size_t o = ((size_t)t * 4 + r) * 64 + lane;
            const double v = (red[o] + red[(size_t)NT * 256 + o]) + (red[(size_t)2 * NT * 256 + o] + red[(size_t)3 * NT * 256 + o]);
            const int i = 16 * t + kg + 4 * r, j = ci;     /* C/D layout of v_mfma_f64_16x16x4_f64 */
            if (i < ncv && j < nxv)
               partials[(size_t)blockIdx.x * nout + (size_t)(j0 + i) + (size_t)(c0 + j) * segs.total] = v;
         }
   }
}

static int dots_mfma_enabled(void) {             /* HIPK_NO_MFMA: measurement knob, read once */
   static int v = -1;
   if (v < 0) v = getenv("HIPK_NO_MFMA") == NULL;
   return v;
}

template <typename T, int VW>
static void dots_launch(hipk_ctx *ctx, dim3 grid, int nxt, const SegArgs &sa, const T *X, int64_t ldX,
      int nx, int64_t m) {
   dim3 block(HIPK_BLOCK);
   switch (nxt) {
   case 1: hipLaunchKernelGGL((dots_kernel<T, 8, 1, VW>), grid, block, 0, ctx->stream, sa, X, ldX, nx, m, ctx->partials); break;
   case 2: hipLaunchKernelGGL((dots_kernel<T, 8, 2, VW>), grid, block, 0, ctx->stream, sa, X, ldX, nx, m, ctx->partials); break;
   case 4: hipLaunchKernelGGL((dots_kernel<T, 8, 4, VW>), grid, block, 0, ctx->stream, sa, X, ldX, nx, m, ctx->partials); break;
   default: hipLaunchKernelGGL((dots_kernel<T, 8, 8, VW>), grid, block, 0, ctx->stream, sa, X, ldX, nx, m, ctx->partials); break;
   }
}

template <typename T>
static int panel_dots_t(hipk_ctx *ctx, int64_t m, const SegArgs &sa, const T *X, int64_t ldX,
      int nx, double *out_dev, int ldout) {
   const int NC = 8;
   int nxt = nx <= 1 ? 1 : nx <= 2 ? 2 : nx <= 4 ? 4 : 8;
   const bool vec = segs_aligned16(sa, sizeof(T)) && aligned16(X, ldX, sizeof(T));
   const int VWm = vec ? (int)vecwidth<T>::value : 1;
   int gx = hipk_grid_for_rows(ctx, m / VWm + 1, HIPK_BLOCK * 2, 4);
   int gy = (sa.total + NC - 1) / NC;
   int gz = (nx + nxt - 1) / nxt;
   /* keep the chip full when the chunk grid is already wide */
   while (gx > 1 && (int64_t)gx * gy * gz > (int64_t)ctx->num_cu * 8) gx = (gx + 1) / 2;
   size_t nout = (size_t)sa.total * nx;
   /* blocks of right-hand columns against more than one chunk of basis columns: wave-per-chunk
    * kernel, the right-hand columns are read once per workgroup */
   const bool wide = (nx >= 4 && sa.total > NC && vec);
   if (wide) {
      const int WAVES = 4;
      gx = hipk_grid_for_rows(ctx, m / VWm + 1, 64 * 4, 8);
      gy = (sa.total + NC * WAVES - 1) / (NC * WAVES);
      nxt = (nx <= 4) ? 4 : 8;
      gz = (nx + nxt - 1) / nxt;
   }
   /* matrix cores for blocks of >= 4 right-hand columns (16-byte aligned panels) */
   const bool mfma = (nx >= 4 && vec && dots_mfma_enabled());
   int nt = 1;
   if (mfma) {
      nt = sa.total <= 16 ? 1 : 2;                 /* 2 tiles: 48 staged columns = 50 KB of LDS */
      gy = (sa.total + 16 * nt - 1) / (16 * nt);
      gz = (nx + 15) / 16;
      static int mbpc = -1;                         /* HIPK_MFMA_BPC: workgroups per CU (measurement knob, read once) */
      if (mbpc < 0) { const char *e = getenv("HIPK_MFMA_BPC"); mbpc = e ? atoi(e) : 3; if (mbpc < 1) mbpc = 3; }      /* 3: 0.50 / 0.71 / 0.66 of HBM at 8 / 16 / 24 basis columns, 2: 0.44 / 0.67 / 0.63 (profiles/r06_zpanel_perf.txt) */
      gx = hipk_grid_for_rows(ctx, m, MF_ROWS, mbpc);
      while (gx > 1 && (int64_t)gx * gy * gz > (int64_t)ctx->num_cu * 2 * mbpc) gx = (gx + 1) / 2;
   }
   if (hipk_reserve_partials(ctx, (size_t)gx * nout)) return -2;
   dim3 grid(gx, gy, gz);
   const int pslot = hipk_prof_begin(HIPK_PROF_DOTS, ctx->stream, (double)m * sizeof(T) * (sa.total + nx));
   if (mfma) {
      const size_t shm = (size_t)(16 * nt + 16) * MF_LDS_STRIDE * sizeof(double);
      if (nt == 1) hipLaunchKernelGGL((dots_mfma_kernel<T, 1>), grid, dim3(HIPK_BLOCK), shm, ctx->stream, sa, X, ldX, nx, m, ctx->partials);
      else hipLaunchKernelGGL((dots_mfma_kernel<T, 2>), grid, dim3(HIPK_BLOCK), shm, ctx->stream, sa, X, ldX, nx, m, ctx->partials);
   } else if (wide) {
      if (nxt == 4) hipLaunchKernelGGL((dots_wide_kernel<T, 8, 4, vecwidth<T>::value, 4>), grid, dim3(256), 0, ctx->stream, sa, X, ldX, nx, m, ctx->partials);
      else hipLaunchKernelGGL((dots_wide_kernel<T, 8, 8, vecwidth<T>::value, 4>), grid, dim3(256), 0, ctx->stream, sa, X, ldX, nx, m, ctx->partials);
   } else if (vec) dots_launch<T, vecwidth<T>::value>(ctx, grid, nxt, sa, X, ldX, nx, m);
   else dots_launch<T, 1>(ctx, grid, nxt, sa, X, ldX, nx, m);
   hipk_prof_end(pslot, ctx->stream);
   HIPK_CHECK(hipGetLastError());
   const size_t span = (size_t)ldout * (nx - 1) + sa.total;      /* from the first result to the last one stored */
   hipLaunchKernelGGL(finalize_ld_kernel, dim3((unsigned)nout), dim3(HIPK_BLOCK), 0, ctx->stream,
         ctx->partials, gx, (int)nout, sa.total, ldout, out_dev, hipk_mirror_of(ctx, out_dev, span), hipk_next_flag(ctx, out_dev, span));
   HIPK_CHECK(hipGetLastError());
   return 0;
}

extern "C" int hipk_panel_dots(hipk_ctx *ctx, hipk_dtype dt, int64_t m, const hipk_seg *segs,
      int nseg, const void *X, int64_t ldX, int nx, double *out_dev, int ldout) {
   if (HIPK_IS_Z(dt)) return hipk_z_panel_dots(ctx, dt, m, segs, nseg, X, ldX, nx, out_dev, ldout);
   SegArgs sa;
   if (pack_segs(segs, nseg, &sa)) return -1;
   if (sa.total == 0 || nx <= 0) return 0;
   if (ldout < sa.total) return -1;
   DISPATCH_RT(dt, return panel_dots_t<T>(ctx, m, sa, (const T *)X, ldX, nx, out_dev, ldout));
}

/* ===================== NN-accumulate: project + norms ========================= */
template <typename T, int NX, int VW>
__global__ void __launch_bounds__(HIPK_BLOCK)
project_kernel(SegArgs segs, const double *__restrict__ coef, int ldcoef, T *X,
      int64_t ldX, T *Xout, int64_t ldXout, int nx, int c0, int64_t m, double *__restrict__ partials, hipk_fin_args fa) {
   typedef lanevec<T, VW> LV;
   __shared__ int s_last;
   __shared__ double scoef[PROJ_MAXCOLS * NX];
   __shared__ const T *sptr[PROJ_MAXCOLS];
   const int total = segs.total;
   const int nxv = min(NX, nx - c0);
   for (int t = threadIdx.x; t < total * NX; t += HIPK_BLOCK) {
      int j = t / NX, c = t % NX;
      scoef[t] = (c < nxv) ? coef[j + (size_t)(c0 + c) * ldcoef] : 0.0;
   }
   for (int j = threadIdx.x; j < total; j += HIPK_BLOCK) sptr[j] = seg_col<T>(segs, j);
   __syncthreads();

   T *xp = X + (size_t)c0 * (size_t)ldX;
   T *op = Xout + (size_t)c0 * (size_t)ldXout;      /* == xp for the in-place form */
   double n2[NX];
#pragma unroll
   for (int c = 0; c < NX; c++) n2[c] = 0.0;

   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   const int64_t mg = m / VW;
   for (int64_t g = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; g < mg; g += stride) {
      double xv[NX][VW];
#pragma unroll
      for (int c = 0; c < NX; c++) {
         if (c < nxv) {
            LV t = ((const LV *)(xp + (size_t)c * ldX))[g];
#pragma unroll
            for (int r = 0; r < VW; r++) xv[c][r] = (double)t.e[r];
         } else {
#pragma unroll
            for (int r = 0; r < VW; r++) xv[c][r] = 0.0;
         }
      }
      int j = 0;
      for (; j + 8 <= total; j += 8) {
         LV a[8];
#pragma unroll
         for (int u = 0; u < 8; u++) a[u] = ldstream<T, VW, 2>(sptr[j + u], g);
#pragma unroll
         for (int u = 0; u < 8; u++)
#pragma unroll
            for (int c = 0; c < NX; c++) {
               const double cf = scoef[(j + u) * NX + c];
#pragma unroll
               for (int r = 0; r < VW; r++) xv[c][r] = fma(-(double)a[u].e[r], cf, xv[c][r]);
            }
      }
      for (; j < total; j++) {
         LV a = ((const LV *)sptr[j])[g];
#pragma unroll
         for (int c = 0; c < NX; c++) {
            const double cf = scoef[j * NX + c];
#pragma unroll
            for (int r = 0; r < VW; r++) xv[c][r] = fma(-(double)a.e[r], cf, xv[c][r]);
         }
      }
#pragma unroll
      for (int c = 0; c < NX; c++)
         if (c < nxv) {
            LV o;
#pragma unroll
            for (int r = 0; r < VW; r++) {
               o.e[r] = (T)xv[c][r];
               n2[c] = fma((double)o.e[r], (double)o.e[r], n2[c]);
            }
            ((LV *)(op + (size_t)c * ldXout))[g] = o;
         }
   }
   if (VW > 1 && blockIdx.x == 0 && threadIdx.x < (unsigned)(m - mg * VW)) {   /* ragged tail rows */
      const int64_t i = mg * VW + threadIdx.x;
      for (int c = 0; c < nxv; c++) {
         double v = (double)xp[i + (size_t)c * ldX];
         for (int j = 0; j < total; j++) v = fma(-(double)sptr[j][i], scoef[j * NX + c], v);
         T o = (T)v;
         op[i + (size_t)c * ldXout] = o;
#pragma unroll
         for (int cc = 0; cc < NX; cc++) if (cc == c) n2[cc] = fma((double)o, (double)o, n2[cc]);
      }
   }
   if (partials) {
      __shared__ double sm[HIPK_BLOCK / HIPK_WAVE][NX];
      const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
      for (int c = 0; c < NX; c++) {
         double v = hipk_wave_sum(n2[c]);
         if (lane == 0) sm[wv][c] = v;
      }
      __syncthreads();
      if (threadIdx.x < nxv)
         hipk_pstore(fa, partials + (size_t)(c0 + threadIdx.x) * gridDim.x + blockIdx.x,
               (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]));
      hipk_inkernel_finalize(partials, nx, gridDim.x, fa, &s_last);
   }
}

/* X <- (X - [segs] coef) * M in ONE pass over X and the basis (M: nx x nx, nx <= NX <= 8): the
 * update and the right-multiplication of a CholQR / SVQB sweep (reference Num_ortho_kernel,
 * ortho.c:963-1072: two GEMMs and a copy through an m x b temporary). */
template <typename T, int NX, int VW>
__global__ void __launch_bounds__(HIPK_BLOCK)
project_mul_kernel(SegArgs segs, const double *__restrict__ coef, int ldcoef, const double *__restrict__ Mr,
      T *X, int64_t ldX, int nx, int64_t m) {
   typedef lanevec<T, VW> LV;
   __shared__ double scoef[PROJ_MAXCOLS * NX];
   __shared__ double sM[NX * NX];
   __shared__ const T *sptr[PROJ_MAXCOLS];
   const int total = segs.total;
   for (int t = threadIdx.x; t < total * NX; t += HIPK_BLOCK) {
      int j = t / NX, c = t % NX;
      scoef[t] = (c < nx) ? coef[j + (size_t)c * ldcoef] : 0.0;
   }
   for (int t = threadIdx.x; t < NX * NX; t += HIPK_BLOCK) {
      int i = t % NX, c = t / NX;                      /* sM[i + c*NX] = M(i, c) */
      sM[t] = (i < nx && c < nx) ? Mr[i + (size_t)c * nx] : 0.0;
   }
   for (int j = threadIdx.x; j < total; j += HIPK_BLOCK) sptr[j] = seg_col<T>(segs, j);
   __syncthreads();
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   const int64_t mg = m / VW;
   for (int64_t g = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; g < mg; g += stride) {
      double xv[NX][VW];
#pragma unroll
      for (int c = 0; c < NX; c++) {
         const LV t = ((const LV *)(X + (size_t)(c < nx ? c : 0) * ldX))[g];
#pragma unroll
         for (int r = 0; r < VW; r++) xv[c][r] = c < nx ? (double)t.e[r] : 0.0;
      }
      int j = 0;
      for (; j + 8 <= total; j += 8) {
         LV a[8];
#pragma unroll
         for (int u = 0; u < 8; u++) a[u] = ((const LV *)sptr[j + u])[g];
#pragma unroll
         for (int u = 0; u < 8; u++)
#pragma unroll
            for (int c = 0; c < NX; c++) {
               const double cf = scoef[(j + u) * NX + c];
#pragma unroll
               for (int r = 0; r < VW; r++) xv[c][r] = fma(-(double)a[u].e[r], cf, xv[c][r]);
            }
      }
      for (; j < total; j++) {
         LV a = ((const LV *)sptr[j])[g];
#pragma unroll
         for (int c = 0; c < NX; c++) {
            const double cf = scoef[j * NX + c];
#pragma unroll
            for (int r = 0; r < VW; r++) xv[c][r] = fma(-(double)a.e[r], cf, xv[c][r]);
         }
      }
#pragma unroll
      for (int c = 0; c < NX; c++)
         if (c < nx) {
            LV o;
#pragma unroll
            for (int r = 0; r < VW; r++) {
               double sacc = 0.0;
#pragma unroll
               for (int i = 0; i < NX; i++) sacc = fma(xv[i][r], sM[i + c * NX], sacc);
               o.e[r] = (T)sacc;
            }
            ((LV *)(X + (size_t)c * ldX))[g] = o;
         }
   }
   if (VW > 1 && blockIdx.x == 0 && threadIdx.x < (unsigned)(m - mg * VW)) {   /* ragged tail rows */
      const int64_t i = mg * VW + threadIdx.x;
      double xv[NX];
      for (int c = 0; c < NX; c++) {
         double v = c < nx ? (double)X[i + (size_t)c * ldX] : 0.0;
         for (int j = 0; j < total; j++) v = fma(-(double)sptr[j][i], scoef[j * NX + c], v);
         xv[c] = v;
      }
      for (int c = 0; c < nx; c++) {
         double sacc = 0.0;
         for (int q = 0; q < NX; q++) sacc = fma(xv[q], sM[q + c * NX], sacc);
         X[i + (size_t)c * ldX] = (T)sacc;
      }
   }
}

template <typename T, int VW>
static int panel_project_mul_v(hipk_ctx *ctx, int64_t m, const SegArgs &sa, const double *coef, int ldcoef,
      const double *Mr, T *X, int64_t ldX, int nx) {
   int gx = hipk_grid_for_rows(ctx, m / VW + 1, HIPK_BLOCK * 2, 4);
   dim3 block(HIPK_BLOCK);
   const int pslot = hipk_prof_begin(HIPK_PROF_PROJECT, ctx->stream, (double)m * sizeof(T) * ((double)sa.total + 2.0 * nx));
   if (nx <= 2) hipLaunchKernelGGL((project_mul_kernel<T, 2, VW>), dim3(gx), block, 0, ctx->stream, sa, coef, ldcoef, Mr, X, ldX, nx, m);
   else if (nx <= 4) hipLaunchKernelGGL((project_mul_kernel<T, 4, VW>), dim3(gx), block, 0, ctx->stream, sa, coef, ldcoef, Mr, X, ldX, nx, m);
   else hipLaunchKernelGGL((project_mul_kernel<T, 8, VW>), dim3(gx), block, 0, ctx->stream, sa, coef, ldcoef, Mr, X, ldX, nx, m);
   hipk_prof_end(pslot, ctx->stream);
   HIPK_CHECK(hipGetLastError());
   return 0;
}

/* X <- (X - [segs] coef) M; returns 1 when the shape is not covered (caller uses the two-pass form) */
extern "C" int hipk_panel_project_mul(hipk_ctx *ctx, hipk_dtype dt, int64_t m, const hipk_seg *segs, int nseg,
      const double *coef_dev, int ldcoef, const double *M_dev, void *X, int64_t ldX, int nx) {
   if (HIPK_IS_Z(dt)) return hipk_z_panel_project(ctx, dt, m, segs, nseg, coef_dev, ldcoef, M_dev, X, ldX, X, ldX, nx, NULL);
   SegArgs sa;
   if (pack_segs(segs, nseg, &sa)) return -1;
   if (nx <= 0) return 0;
   if (nx > 8 || sa.total > PROJ_MAXCOLS) return 1;
   const size_t es = hipk_elem_size(dt);
   const bool vec = segs_aligned16(sa, es) && aligned16(X, ldX, es);
   DISPATCH_RT(dt, return vec ? panel_project_mul_v<T, vecwidth<T>::value>(ctx, m, sa, coef_dev, ldcoef, M_dev, (T *)X, ldX, nx) : panel_project_mul_v<T, 1>(ctx, m, sa, coef_dev, ldcoef, M_dev, (T *)X, ldX, nx));
}

template <typename T, int VW>
static int panel_project_v(hipk_ctx *ctx, int64_t m, const SegArgs &sa, const double *coef,
      int ldcoef, T *X, int64_t ldX, T *Xout, int64_t ldXout, int nx, double *nrm2_dev) {
   int gx = hipk_grid_for_rows(ctx, m / VW + 1, HIPK_BLOCK * 2, 4);
   if (nrm2_dev && hipk_reserve_partials(ctx, (size_t)gx * nx)) return -2;
   dim3 block(HIPK_BLOCK);
   /* one launch covers all columns: its last workgroup finalises the norms itself */
   hipk_fin_args fa;
   memset(&fa, 0, sizeof(fa));
   /* the tail of a block-size-1 iteration (hipk_tail_defer): the partial sums of |t|^2 stay where the operator launch and
    * hipk_tail_finish add them up themselves — no second-stage launch here */
   const bool defer = nrm2_dev && nx == 1 && (ctx->tail_want & HIPK_TAIL_NORM) && ctx->tail_np2 == 0 && gx <= HIPK_TAIL_MAXPART;
   if (!defer && nrm2_dev && (nx == 1 || nx == 2 || nx == 4 || nx == 8)) fa = hipk_make_fin(ctx, nrm2_dev, HIPK_FIN_PROJECT, gx, nx);
   double *part = defer ? ctx->tailp : (nrm2_dev ? ctx->partials : NULL);      /* after hipk_make_fin: it may have grown the buffer */
   const int pslot = hipk_prof_begin(HIPK_PROF_PROJECT, ctx->stream, (double)m * sizeof(T) * ((double)sa.total * ((nx + 7) / 8) + 2.0 * nx));
   for (int c0 = 0; c0 < nx;) {
      int rem = nx - c0;
      int step;
      if (rem >= 8) { step = 8; hipLaunchKernelGGL((project_kernel<T, 8, VW>), dim3(gx), block, 0, ctx->stream, sa, coef, ldcoef, X, ldX, Xout, ldXout, nx, c0, m, part, fa); }
      else if (rem >= 4) { step = 4; hipLaunchKernelGGL((project_kernel<T, 4, VW>), dim3(gx), block, 0, ctx->stream, sa, coef, ldcoef, X, ldX, Xout, ldXout, nx, c0, m, part, fa); }
      else if (rem >= 2) { step = 2; hipLaunchKernelGGL((project_kernel<T, 2, VW>), dim3(gx), block, 0, ctx->stream, sa, coef, ldcoef, X, ldX, Xout, ldXout, nx, c0, m, part, fa); }
      else { step = 1; hipLaunchKernelGGL((project_kernel<T, 1, VW>), dim3(gx), block, 0, ctx->stream, sa, coef, ldcoef, X, ldX, Xout, ldXout, nx, c0, m, part, fa); }
      HIPK_CHECK(hipGetLastError());
      c0 += step;
   }
   hipk_prof_end(pslot, ctx->stream);
   if (defer) { ctx->tail_np2 = gx; ctx->tail_norm2_out = nrm2_dev; return 0; }
   if (nrm2_dev && !fa.enabled) return hipk_finalize_partials_t(ctx, ctx->partials, gx, nx, nrm2_dev);
   return 0;
}

template <typename T>
static int panel_project_t(hipk_ctx *ctx, int64_t m, const SegArgs &sa, const double *coef,
      int ldcoef, T *X, int64_t ldX, T *Xout, int64_t ldXout, int nx, double *nrm2_dev) {
   if (sa.total > PROJ_MAXCOLS) return -1;
   if (segs_aligned16(sa, sizeof(T)) && aligned16(X, ldX, sizeof(T)) && aligned16(Xout, ldXout, sizeof(T)))
      return panel_project_v<T, vecwidth<T>::value>(ctx, m, sa, coef, ldcoef, X, ldX, Xout, ldXout, nx, nrm2_dev);
   return panel_project_v<T, 1>(ctx, m, sa, coef, ldcoef, X, ldX, Xout, ldXout, nx, nrm2_dev);
}

extern "C" int hipk_panel_project_to(hipk_ctx *ctx, hipk_dtype dt, int64_t m, const hipk_seg *segs,
      int nseg, const double *coef_dev, int ldcoef, const void *X, int64_t ldX, void *Xout, int64_t ldXout,
      int nx, double *nrm2_dev) {
   if (HIPK_IS_Z(dt)) return hipk_z_panel_project(ctx, dt, m, segs, nseg, coef_dev, ldcoef, NULL, X, ldX, Xout, ldXout, nx, nrm2_dev);
   SegArgs sa;
   if (pack_segs(segs, nseg, &sa)) return -1;
   if (nx <= 0) return 0;
   if (sa.total > PROJ_MAXCOLS) {
      /* more columns than one launch stages in LDS: project window by window (the operation
       * is a sum over columns); the first window reads X, the later ones update Xout in place;
       * the norms come from the last window */
      const size_t es = hipk_elem_size(dt);
      for (int w0 = 0; w0 < sa.total; w0 += PROJ_MAXCOLS) {
         const int wn = sa.total - w0 < PROJ_MAXCOLS ? sa.total - w0 : PROJ_MAXCOLS;
         hipk_seg sub[HIPK_MAX_SEGS];
         int ns = 0, c = 0;
         for (int q = 0; q < HIPK_MAX_SEGS; q++) {
            const int lo = w0 > c ? w0 : c, hi = (w0 + wn < c + sa.n[q]) ? w0 + wn : c + sa.n[q];
            if (hi > lo) {
               sub[ns].base = (char *)sa.base[q] + (size_t)(lo - c) * (size_t)sa.ld[q] * es;
               sub[ns].ld = sa.ld[q]; sub[ns].ncols = hi - lo; ns++;
            }
            c += sa.n[q];
         }
         int rc = hipk_panel_project_to(ctx, dt, m, sub, ns, coef_dev + w0, ldcoef, w0 == 0 ? X : Xout, w0 == 0 ? ldX : ldXout,
               Xout, ldXout, nx, (w0 + wn >= sa.total) ? nrm2_dev : NULL);
         if (rc) return rc;
      }
      return 0;
   }
   DISPATCH_RT(dt, return panel_project_t<T>(ctx, m, sa, coef_dev, ldcoef, (T *)X, ldX, (T *)Xout, ldXout, nx, nrm2_dev));
}

extern "C" int hipk_panel_project(hipk_ctx *ctx, hipk_dtype dt, int64_t m, const hipk_seg *segs,
      int nseg, const double *coef_dev, int ldcoef, void *X, int64_t ldX, int nx,
      double *nrm2_dev) {
   return hipk_panel_project_to(ctx, dt, m, segs, nseg, coef_dev, ldcoef, X, ldX, X, ldX, nx, nrm2_dev);
}

/* W <- W - [segs] coef, then out = [x'w | v'w | v'x] for the updated W: the projection of (A - shift) d against the locked
 * vectors (the reference's apply_projected_matrix, inner_solve.c:853-880, Num_gemm + Num_dist_dots) and the three inner
 * products of the block QMR step in ONE pass — the projected panel used to be written by project_kernel and read back by
 * triple_dots_kernel.  Same arithmetic as that pair of launches in the same order (coefficients applied with one fma each in
 * column order; a thread walks the rows triple_dots_kernel gives it, so every partial sum is that kernel's): identical bits,
 * one read of nx columns and one launch less per inner step (round 6). */
template <typename T, int NX>
__global__ void __launch_bounds__(HIPK_BLOCK)
project_triple_kernel(SegArgs segs, const double *__restrict__ coef, int ldcoef, T *__restrict__ Wv, int64_t ldW,
      const T *__restrict__ X, int64_t ldX, const T *__restrict__ Vv, int64_t ldV, int nx, int64_t m, double *__restrict__ partials) {
   __shared__ double scoef[PROJ_MAXCOLS * NX];
   __shared__ const T *sptr[PROJ_MAXCOLS];
   __shared__ double sm[HIPK_BLOCK / HIPK_WAVE][3][NX];
   const int total = segs.total;
   for (int t = threadIdx.x; t < total * NX; t += HIPK_BLOCK) {
      const int j = t / NX, c = t % NX;
      scoef[t] = (c < nx) ? coef[j + (size_t)c * ldcoef] : 0.0;
   }
   for (int j = threadIdx.x; j < total; j += HIPK_BLOCK) sptr[j] = seg_col<T>(segs, j);
   __syncthreads();
   double a[NX], b[NX], d[NX];
#pragma unroll
   for (int c = 0; c < NX; c++) { a[c] = 0.0; b[c] = 0.0; d[c] = 0.0; }
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride) {
      double wv[NX], xv[NX], vv[NX];
#pragma unroll
      for (int c = 0; c < NX; c++) {
         const int cc = c < nx ? c : 0;
         wv[c] = (double)Wv[i + (size_t)cc * ldW];
         xv[c] = (double)X[i + (size_t)cc * ldX];
         vv[c] = (double)Vv[i + (size_t)cc * ldV];
      }
      int j = 0;
      for (; j + 8 <= total; j += 8) {
         double q[8];
#pragma unroll
         for (int u = 0; u < 8; u++) q[u] = (double)__builtin_nontemporal_load(sptr[j + u] + i);
#pragma unroll
         for (int u = 0; u < 8; u++)
#pragma unroll
            for (int c = 0; c < NX; c++) wv[c] = fma(-q[u], scoef[(j + u) * NX + c], wv[c]);
      }
      for (; j < total; j++) {
         const double q = (double)sptr[j][i];
#pragma unroll
         for (int c = 0; c < NX; c++) wv[c] = fma(-q, scoef[j * NX + c], wv[c]);
      }
#pragma unroll
      for (int c = 0; c < NX; c++)
         if (c < nx) {
            const T o = (T)wv[c];
            Wv[i + (size_t)c * ldW] = o;
            const double wi = (double)o;
            a[c] = fma(xv[c], wi, a[c]); b[c] = fma(vv[c], wi, b[c]); d[c] = fma(vv[c], xv[c], d[c]);
         }
   }
   const int lane = threadIdx.x & 63, wvn = threadIdx.x >> 6;
#pragma unroll
   for (int c = 0; c < NX; c++) {
      const double ta = hipk_wave_sum(a[c]), tb = hipk_wave_sum(b[c]), td = hipk_wave_sum(d[c]);
      if (lane == 0) { sm[wvn][0][c] = ta; sm[wvn][1][c] = tb; sm[wvn][2][c] = td; }
   }
   __syncthreads();
   for (int t = threadIdx.x; t < 3 * nx; t += HIPK_BLOCK) {
      const int w = t / nx, c = t % nx;
      partials[(size_t)blockIdx.x * 3 * nx + w * nx + c] = (sm[0][w][c] + sm[1][w][c]) + (sm[2][w][c] + sm[3][w][c]);
   }
}

extern "C" int hipk_project_triple_dots(hipk_ctx *ctx, hipk_dtype dt, int64_t m, const hipk_seg *segs, int nseg, const double *coef_dev,
      int ldcoef, void *W, int64_t ldW, int nx, const void *X, int64_t ldX, const void *V, int64_t ldV, double *out_dev) {
   if (nx <= 0) return 0;
   SegArgs sa;
   if (HIPK_IS_Z(dt) || pack_segs(segs, nseg, &sa) || nx > 8 || sa.total > PROJ_MAXCOLS || sa.total <= 0) return 1;   /* not covered: the caller runs the two launches */
   int gx = hipk_grid_for_rows(ctx, m, HIPK_BLOCK * 4, 4);        /* = hipk_triple_dots: the same partial sums */
   if (hipk_reserve_partials(ctx, (size_t)gx * 3 * nx)) return -2;
   {
      hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)sa.total + 4.0 * nx));
#define PTK(NXV) DISPATCH_RT(dt, \
         hipLaunchKernelGGL((project_triple_kernel<T, NXV>), dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, sa, coef_dev, ldcoef, (T *)W, ldW, (const T *)X, ldX, (const T *)V, ldV, nx, m, ctx->partials))
      if (nx <= 2) { PTK(2); } else if (nx <= 4) { PTK(4); } else { PTK(8); }
#undef PTK
      HIPK_CHECK(hipGetLastError());
   }
   return hipk_finalize_partials(ctx, ctx->partials, gx, 3 * nx, out_dev);
}
