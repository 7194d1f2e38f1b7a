/* hipk_amg.hip — device pieces of the aggregation algebraic multigrid preconditioner for CSR operators (gfx950).
 *
 * One V-cycle (primme_amd_amg_precond in amd_operator.hip; DESIGN.md, "Aggregation algebraic multigrid preconditioner") runs
 * the level operators through hipk_csr_matvec and, between the products, these passes over panels of vectors:
 *   amg_update_kernel    Out = cy Yk + cp Yprev + dinv o (cx X + cw W): a step of the Chebyshev iteration for D^-1 M_l with
 *                        W = M_l Yk, or (dinv = NULL, cx = 1, cw = -1) the residual; row-local
 *   amg_restrict_kernel  C[j] = sum of F over the rows of aggregate j (P' F for the 0/1 matrix P of the aggregate map)
 *   amg_prolong_kernel   Y[i] += over C[agg[i]]  (Y += over P C)
 *   amg_dense_kernel     Y = G X for the dense inverse G of the last level, at most PRIMME_AMD_AMG_DENSE_ROWS rows
 *   amg_csr_kernel       Out = T In or Out += T In for a CSR matrix T with double values: the restriction (T = P') and the
 *                        interpolation (T = P) of smoothed aggregation, where P has several entries per row
 * A lane owns VW consecutive elements of the streamed panel (VW = 16 bytes when base and leading dimension of every streamed
 * panel allow it, one element where not); what is indexed through a map (the rows of an aggregate, the aggregate of a row) is
 * an element load.  Arithmetic in double whatever T is, one rounding per stored element.  No atomics: every sum has one
 * order, so a result is the same from run to run.  blockIdx.y = column.  The entry points check sizes and pointers; the
 * index arrays are the library's own (made from the host plan) and are trusted.  No reference counterpart. */
#include "hipk_internal.h"
#include "primme_amd_io.h"   /* PRIMME_AMD_AMG_DENSE_ROWS */

/* an aggregate of at most AMG_LANE_ROWS rows is summed by its lane, a longer one by the whole wave */
#define AMG_LANE_ROWS 64

template <typename T, int VW> struct alignas(sizeof(T) * VW) amg_pack { T v[VW]; };
struct alignas(16) amg_d2 { double v[2]; };

template <typename T, int VW>
__global__ void __launch_bounds__(HIPK_BLOCK)
amg_update_kernel(int64_t m, hipk_cheb_coef cf, const double *__restrict__ dinv, const T *X, int64_t ldx, const T *W, int64_t ldw,
      const T *Yk, int64_t ldk, const T *Yp, int64_t ldp, T *Out, int64_t ldo) {
   typedef amg_pack<T, VW> P;
   const int c = blockIdx.y;
   const double cy = cf.cy[c], cp = cf.cp[c], cx = cf.cx[c], cw = cf.cw[c];
   const T *x = X + (size_t)c * ldx, *w = W ? W + (size_t)c * ldw : NULL, *yk = Yk ? Yk + (size_t)c * ldk : NULL,
           *yp = Yp ? Yp + (size_t)c * ldp : NULL;
   T *out = Out + (size_t)c * ldo;
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK, gid = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x;
   const int64_t nv = m / VW;
   for (int64_t i = gid; i < nv; i += stride) {
      const P px = ((const P *)x)[i];
      P pw = px, pk = px, pp = px, po;
      double dv[VW];
#pragma unroll
      for (int e = 0; e < VW; e++) dv[e] = 1.0;
      if (dinv) {
         if (VW == 1) dv[0] = dinv[i];
         else {
#pragma unroll
            for (int e = 0; e < VW; e += 2) {
               const amg_d2 d = ((const amg_d2 *)dinv)[(i * VW + e) / 2];
               dv[e] = d.v[0]; dv[e + 1 < VW ? e + 1 : e] = d.v[1];
            }
         }
      }
      if (w) pw = ((const P *)w)[i];
      if (yk) pk = ((const P *)yk)[i];
      if (yp) pp = ((const P *)yp)[i];
#pragma unroll
      for (int e = 0; e < VW; e++) {
         double r = cx * (double)px.v[e];
         if (w) r = fma(cw, (double)pw.v[e], r);
         double s = dv[e] * r;
         if (yk) s = fma(cy, (double)pk.v[e], s);
         if (yp) s = fma(cp, (double)pp.v[e], s);
         po.v[e] = (T)s;
      }
      ((P *)out)[i] = po;
   }
   /* the rows past the last full access */
   for (int64_t i = nv * VW + gid; i < m; i += stride) {
      double r = cx * (double)x[i];
      if (w) r = fma(cw, (double)w[i], r);
      double s = (dinv ? dinv[i] : 1.0) * r;
      if (yk) s = fma(cy, (double)yk[i], s);
      if (yp) s = fma(cp, (double)yp[i], s);
      out[i] = (T)s;
   }
}

/* A wave takes 64 VW consecutive aggregates per trip, lane l the VW from base + l VW on.  An aggregate of at most
 * AMG_LANE_ROWS rows is added up by its lane, rows ascending.  A longer one is then taken by the whole wave: lane l adds the
 * rows first + l, first + l + 64, ... in that order, and the 64 partial sums are folded by the xor butterfly 32, 16, ... 1
 * (a + b = b + a exactly, so every lane holds the same bits).  The trip loop and the loop over the long aggregates are
 * wave-uniform: all 64 lanes reach every ballot and shuffle. */
template <typename T, int VW>
__global__ void __launch_bounds__(HIPK_BLOCK)
amg_restrict_kernel(int64_t nc, const int32_t *__restrict__ aggptr, const int32_t *__restrict__ aggrows, const T *F, int64_t ldf,
      T *C, int64_t ldc) {
   typedef amg_pack<T, VW> P;
   const T *__restrict__ f = F + (size_t)blockIdx.y * ldf;
   T *cc = C + (size_t)blockIdx.y * ldc;
   const int lane = threadIdx.x & (HIPK_WAVE - 1);
   const int64_t nwaves = (int64_t)gridDim.x * (HIPK_BLOCK / HIPK_WAVE);
   const int64_t wave = (int64_t)blockIdx.x * (HIPK_BLOCK / HIPK_WAVE) + (threadIdx.x / HIPK_WAVE);
   const int64_t per = (int64_t)HIPK_WAVE * VW;
   for (int64_t base = wave * per; base < nc; base += nwaves * per) {
      const int64_t j0 = base + (int64_t)lane * VW;
      double s[VW];
      int32_t p0[VW], p1[VW];
#pragma unroll
      for (int e = 0; e < VW; e++) {
         const int64_t j = j0 + e;
         p0[e] = p1[e] = 0;
         if (j < nc) { p0[e] = aggptr[j]; p1[e] = aggptr[j + 1]; }
         s[e] = 0.0;
         if (p1[e] - p0[e] <= AMG_LANE_ROWS)
            for (int32_t p = p0[e]; p < p1[e]; p++) s[e] += (double)f[aggrows[p]];
      }
#pragma unroll
      for (int e = 0; e < VW; e++) {
         unsigned long long mask = __ballot(p1[e] - p0[e] > AMG_LANE_ROWS);
         while (mask) {
            const int src = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const int32_t q0 = __shfl(p0[e], src), q1 = __shfl(p1[e], src);
            double t = 0.0;
            for (int32_t p = q0 + lane; p < q1; p += HIPK_WAVE) t += (double)f[aggrows[p]];
            for (int o = HIPK_WAVE / 2; o > 0; o >>= 1) t += __shfl_xor(t, o);
            if (lane == src) s[e] = t;
         }
      }
      if (VW > 1 && j0 + VW <= nc) {
         P po;
#pragma unroll
         for (int e = 0; e < VW; e++) po.v[e] = (T)s[e];
         *(P *)(cc + j0) = po;
      } else {
#pragma unroll
         for (int e = 0; e < VW; e++)
            if (j0 + e < nc) cc[j0 + e] = (T)s[e];
      }
   }
}

template <typename T, int VW>
__global__ void __launch_bounds__(HIPK_BLOCK)
amg_prolong_kernel(int64_t nf, double over, const int32_t *__restrict__ agg, const T *C, int64_t ldc, T *Y, int64_t ldy) {
   typedef amg_pack<T, VW> P;
   const T *__restrict__ cc = C + (size_t)blockIdx.y * ldc;
   T *y = Y + (size_t)blockIdx.y * ldy;
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK, gid = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x;
   const int64_t nv = nf / VW;
   for (int64_t i = gid; i < nv; i += stride) {
      P py = ((const P *)y)[i];
#pragma unroll
      for (int e = 0; e < VW; e++) py.v[e] = (T)fma(over, (double)cc[agg[i * VW + e]], (double)py.v[e]);
      ((P *)y)[i] = py;
   }
   for (int64_t i = nv * VW + gid; i < nf; i += stride) y[i] = (T)fma(over, (double)cc[agg[i]], (double)y[i]);
}

/* Out = T In (ACC = 0) or Out += T In (ACC = 1) for a CSR matrix T with double values: the transfers of smoothed aggregation,
 * T = R_l = P_l' (restriction) and T = P_l (interpolation).  The rows are dealt as amg_restrict_kernel deals the aggregates:
 * a wave takes 64 VW consecutive rows per trip, lane l the VW from base + l VW on; a row of at most AMG_LANE_ROWS entries is
 * summed by its lane, positions ascending, a longer one by the whole wave, lane l the positions first + l, first + l + 64, ...
 * and the 64 partial sums folded by the xor butterfly.  The sum is in double; with ACC the lane's VW elements of Out are
 * loaded in one access, added in double, and the result rounded once.  Wave-uniform trip and long-row loops. */
template <typename T, int VW, int ACC>
__global__ void __launch_bounds__(HIPK_BLOCK)
amg_csr_kernel(int64_t nrows, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colind, const double *__restrict__ values,
      const T *In, int64_t ldin, T *Out, int64_t ldout) {
   typedef amg_pack<T, VW> P;
   const T *__restrict__ in = In + (size_t)blockIdx.y * ldin;
   T *out = Out + (size_t)blockIdx.y * ldout;
   const int lane = threadIdx.x & (HIPK_WAVE - 1);
   const int64_t nwaves = (int64_t)gridDim.x * (HIPK_BLOCK / HIPK_WAVE);
   const int64_t wave = (int64_t)blockIdx.x * (HIPK_BLOCK / HIPK_WAVE) + (threadIdx.x / HIPK_WAVE);
   const int64_t per = (int64_t)HIPK_WAVE * VW;
   for (int64_t base = wave * per; base < nrows; base += nwaves * per) {
      const int64_t j0 = base + (int64_t)lane * VW;
      double s[VW];
      int32_t p0[VW], p1[VW];
#pragma unroll
      for (int e = 0; e < VW; e++) {
         const int64_t j = j0 + e;
         p0[e] = p1[e] = 0;
         if (j < nrows) { p0[e] = rowptr[j]; p1[e] = rowptr[j + 1]; }
         s[e] = 0.0;
         if (p1[e] - p0[e] <= AMG_LANE_ROWS)
            for (int32_t p = p0[e]; p < p1[e]; p++) s[e] = fma(values[p], (double)in[colind[p]], s[e]);
      }
#pragma unroll
      for (int e = 0; e < VW; e++) {
         unsigned long long mask = __ballot(p1[e] - p0[e] > AMG_LANE_ROWS);
         while (mask) {
            const int src = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const int32_t q0 = __shfl(p0[e], src), q1 = __shfl(p1[e], src);
            double t = 0.0;
            for (int32_t p = q0 + lane; p < q1; p += HIPK_WAVE) t = fma(values[p], (double)in[colind[p]], t);
            for (int o = HIPK_WAVE / 2; o > 0; o >>= 1) t += __shfl_xor(t, o);
            if (lane == src) s[e] = t;
         }
      }
      if (VW > 1 && j0 + VW <= nrows) {
         P po;
         if (ACC) po = *(const P *)(out + j0);
#pragma unroll
         for (int e = 0; e < VW; e++) po.v[e] = (T)(ACC ? s[e] + (double)po.v[e] : s[e]);
         *(P *)(out + j0) = po;
      } else {
#pragma unroll
         for (int e = 0; e < VW; e++)
            if (j0 + e < nrows) out[j0 + e] = (T)(ACC ? s[e] + (double)out[j0 + e] : s[e]);
      }
   }
}

/* one workgroup per column: the column of X in LDS, thread i row i of G X with the terms added in ascending order of the
 * column index; G is symmetric, so its row i is read as column i and consecutive threads read consecutive addresses */
template <typename T>
__global__ void __launch_bounds__(PRIMME_AMD_AMG_DENSE_ROWS)
amg_dense_kernel(int n, const double *__restrict__ G, const T *X, int64_t ldx, T *Y, int64_t ldy) {
   __shared__ double xs[PRIMME_AMD_AMG_DENSE_ROWS];
   const int i = threadIdx.x;
   const T *x = X + (size_t)blockIdx.x * ldx;
   T *y = Y + (size_t)blockIdx.x * ldy;
   if (i < n) xs[i] = (double)x[i];
   __syncthreads();
   if (i >= n) return;
   double s = 0.0;
   for (int j = 0; j < n; j++) s = fma(G[(size_t)j * n + i], xs[j], s);
   y[i] = (T)s;
}

/* ---- launchers ------------------------------------------------------------------------------------------------------- */
static int amg_num_cu(void) {
   static int num_cu = 0;                      /* launch geometry only: read the device once */
   if (num_cu == 0) {
      int dev = 0, n = 0;
      if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) num_cu = n;
      else num_cu = 256;
   }
   return num_cu;
}
static bool amg_al16(const void *p, int64_t ld, size_t es) { return !p || (((uintptr_t)p & 15) == 0 && ((size_t)ld * es) % 16 == 0); }
/* workgroups for m elements, `per` of them per workgroup and trip, two trips, at most eight workgroups per compute unit */
static unsigned amg_grid(int64_t m, int64_t per) {
   const int64_t cap = (int64_t)amg_num_cu() * 8;
   int64_t gx = (m + 2 * per - 1) / (2 * per);
   if (gx > cap) gx = cap;
   return (unsigned)(gx < 1 ? 1 : gx);
}

extern "C" int hipk_amg_smooth_update(void *hip_stream, hipk_dtype dt, int64_t m, int nx, const hipk_cheb_coef *coef, const double *dinv,
      const void *X, int64_t ldx, const void *W, int64_t ldw, const void *Yk, int64_t ldk, const void *Yprev, int64_t ldp, void *Out, int64_t ldo) {
   if (dt != HIPK_F64 && dt != HIPK_F32) return -44;
   if (nx <= 0 || m == 0) return 0;
   if (m < 0 || nx > HIPK_CHEB_MAXCOLS || !coef || !X || !Out) return -1;
   hipStream_t st = (hipStream_t)hip_stream;
   hipk_prof_scope ps_(HIPK_PROF_VEC, st, hipk_stream_bytes(dt, m, (double)nx * (2 + (W != NULL) + (Yk != NULL) + (Yprev != NULL))) + (dinv ? 8.0 * m * nx : 0.0));
   DISPATCH_RT(dt, {
      constexpr int VW = 16 / sizeof(T);
      const bool vec = amg_al16(X, ldx, sizeof(T)) && amg_al16(W, ldw, sizeof(T)) && amg_al16(Yk, ldk, sizeof(T)) &&
                       amg_al16(Yprev, ldp, sizeof(T)) && amg_al16(Out, ldo, sizeof(T)) && amg_al16(dinv, 2, 8);
      const dim3 grid(amg_grid(m, (int64_t)HIPK_BLOCK * (vec ? VW : 1)), nx);
      if (vec) hipLaunchKernelGGL((amg_update_kernel<T, VW>), grid, dim3(HIPK_BLOCK), 0, st, m, *coef, dinv, (const T *)X, ldx, (const T *)W, ldw,
            (const T *)Yk, ldk, (const T *)Yprev, ldp, (T *)Out, ldo);
      else hipLaunchKernelGGL((amg_update_kernel<T, 1>), grid, dim3(HIPK_BLOCK), 0, st, m, *coef, dinv, (const T *)X, ldx, (const T *)W, ldw,
            (const T *)Yk, ldk, (const T *)Yprev, ldp, (T *)Out, ldo);
   });
   HIPK_CHECK(hipGetLastError());
   return 0;
}

extern "C" int hipk_amg_restrict(void *hip_stream, hipk_dtype dt, int64_t nf, int64_t nc, const int32_t *aggptr, const int32_t *aggrows, int nx,
      const void *F, int64_t ldf, void *C, int64_t ldc) {
   if (dt != HIPK_F64 && dt != HIPK_F32) return -44;
   if (nx <= 0) return 0;
   if (nf < 1 || nc < 1 || nc > nf || nf > INT32_MAX || nx > HIPK_CHEB_MAXCOLS || !aggptr || !aggrows || !F || !C || F == C) return -1;
   hipStream_t st = (hipStream_t)hip_stream;
   hipk_prof_scope ps_(HIPK_PROF_VEC, st, hipk_stream_bytes(dt, nf + nc, (double)nx) + 4.0 * (nf + nc) * nx);
   DISPATCH_RT(dt, {
      constexpr int VW = 16 / sizeof(T);
      const bool vec = amg_al16(C, ldc, sizeof(T));                /* the stored panel; F is read row by row */
      const dim3 grid(amg_grid(nc, (int64_t)HIPK_BLOCK * (vec ? VW : 1)), nx);
      if (vec) hipLaunchKernelGGL((amg_restrict_kernel<T, VW>), grid, dim3(HIPK_BLOCK), 0, st, nc, aggptr, aggrows, (const T *)F, ldf, (T *)C, ldc);
      else hipLaunchKernelGGL((amg_restrict_kernel<T, 1>), grid, dim3(HIPK_BLOCK), 0, st, nc, aggptr, aggrows, (const T *)F, ldf, (T *)C, ldc);
   });
   HIPK_CHECK(hipGetLastError());
   return 0;
}

extern "C" int hipk_amg_prolong_add(void *hip_stream, hipk_dtype dt, int64_t nf, int64_t nc, const int32_t *agg, double over, int nx,
      const void *C, int64_t ldc, void *Y, int64_t ldy) {
   if (dt != HIPK_F64 && dt != HIPK_F32) return -44;
   if (nx <= 0) return 0;
   if (nf < 1 || nc < 1 || nc > nf || nf > INT32_MAX || nx > HIPK_CHEB_MAXCOLS || !agg || !C || !Y || C == Y) return -1;
   hipStream_t st = (hipStream_t)hip_stream;
   hipk_prof_scope ps_(HIPK_PROF_VEC, st, hipk_stream_bytes(dt, 2 * nf + nc, (double)nx) + 4.0 * nf * nx);
   DISPATCH_RT(dt, {
      constexpr int VW = 16 / sizeof(T);
      const bool vec = amg_al16(Y, ldy, sizeof(T));                /* the updated panel; C is read through the map */
      const dim3 grid(amg_grid(nf, (int64_t)HIPK_BLOCK * (vec ? VW : 1)), nx);
      if (vec) hipLaunchKernelGGL((amg_prolong_kernel<T, VW>), grid, dim3(HIPK_BLOCK), 0, st, nf, over, agg, (const T *)C, ldc, (T *)Y, ldy);
      else hipLaunchKernelGGL((amg_prolong_kernel<T, 1>), grid, dim3(HIPK_BLOCK), 0, st, nf, over, agg, (const T *)C, ldc, (T *)Y, ldy);
   });
   HIPK_CHECK(hipGetLastError());
   return 0;
}

extern "C" int hipk_amg_csr_apply(void *hip_stream, hipk_dtype dt, int64_t nrows, int64_t ncols, const int32_t *rowptr, const int32_t *colind,
      const double *values, int accumulate, int nx, const void *In, int64_t ldin, void *Out, int64_t ldout) {
   if (dt != HIPK_F64 && dt != HIPK_F32) return -44;
   if (nx <= 0) return 0;
   if (nrows < 1 || ncols < 1 || nrows > INT32_MAX || ncols > INT32_MAX || nx > HIPK_CHEB_MAXCOLS || !rowptr || !colind || !values ||
       !In || !Out || In == Out) return -1;
   hipStream_t st = (hipStream_t)hip_stream;
   hipk_prof_scope ps_(HIPK_PROF_VEC, st, hipk_stream_bytes(dt, (accumulate ? 2 : 1) * nrows + ncols, (double)nx) + 4.0 * nrows * nx);
   DISPATCH_RT(dt, {
      constexpr int VW = 16 / sizeof(T);
      const bool vec = amg_al16(Out, ldout, sizeof(T));            /* the stored panel; In is read through the column indices */
      const dim3 grid(amg_grid(nrows, (int64_t)HIPK_BLOCK * (vec ? VW : 1)), nx);
      if (vec && accumulate) hipLaunchKernelGGL((amg_csr_kernel<T, VW, 1>), grid, dim3(HIPK_BLOCK), 0, st, nrows, rowptr, colind, values, (const T *)In, ldin, (T *)Out, ldout);
      else if (vec) hipLaunchKernelGGL((amg_csr_kernel<T, VW, 0>), grid, dim3(HIPK_BLOCK), 0, st, nrows, rowptr, colind, values, (const T *)In, ldin, (T *)Out, ldout);
      else if (accumulate) hipLaunchKernelGGL((amg_csr_kernel<T, 1, 1>), grid, dim3(HIPK_BLOCK), 0, st, nrows, rowptr, colind, values, (const T *)In, ldin, (T *)Out, ldout);
      else hipLaunchKernelGGL((amg_csr_kernel<T, 1, 0>), grid, dim3(HIPK_BLOCK), 0, st, nrows, rowptr, colind, values, (const T *)In, ldin, (T *)Out, ldout);
   });
   HIPK_CHECK(hipGetLastError());
   return 0;
}

extern "C" int hipk_amg_dense_apply(void *hip_stream, hipk_dtype dt, int n, const double *G, int nx, const void *X, int64_t ldx, void *Y, int64_t ldy) {
   if (dt != HIPK_F64 && dt != HIPK_F32) return -44;
   if (nx <= 0) return 0;
   if (n < 1 || n > PRIMME_AMD_AMG_DENSE_ROWS || nx > HIPK_CHEB_MAXCOLS || !G || !X || !Y) return -1;
   hipStream_t st = (hipStream_t)hip_stream;
   hipk_prof_scope ps_(HIPK_PROF_VEC, st, hipk_stream_bytes(dt, 2 * (int64_t)n, (double)nx) + 8.0 * n * n);
   DISPATCH_RT(dt, {
      hipLaunchKernelGGL((amg_dense_kernel<T>), dim3(nx), dim3(PRIMME_AMD_AMG_DENSE_ROWS), 0, st, n, G, (const T *)X, ldx, (T *)Y, ldy);
   });
   HIPK_CHECK(hipGetLastError());
   return 0;
}
