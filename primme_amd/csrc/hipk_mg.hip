/* hipk_mg.hip — device pieces of the geometric multigrid preconditioner for grid Laplacians (gfx950).
 *
 * One V-cycle (primme_amd_multigrid_precond in amd_operator.hip; DESIGN.md, "Geometric multigrid preconditioner") is made of
 * three matrix-free passes over panels of grid vectors, x fastest:
 *   mg_step_kernel      Out = cx X + cy Yk + cp Yprev + cw (sum_d w_d L_d Yk): a step of the Chebyshev smoother or the residual
 *                       b - M y of M = scale sum_d w_d L_d + shift I, the constants folded into the coefficients
 *   mg_restrict_kernel  C = R F, full weighting (1/4, 1/2, 1/4 per coarsened dimension), coarse point j on fine point 2 j + 1
 *   mg_prolong_kernel   Y += P C, linear interpolation
 * All three stream: a lane owns VW consecutive points of the FLAT vector (VW = 16 bytes when base and leading dimension of
 * every streamed panel allow it, one element where not), finds its grid position with two 32-bit divisions per trip and steps
 * it from point to point, so a 16-byte access may lie across the end of a grid row.  What a point needs from other points —
 * the six neighbours, the 27 fine points of a restriction, the 8 coarse points of an interpolation — are element loads that
 * the neighbouring lanes' streamed accesses have brought into cache; no LDS.  Arithmetic in double whatever T is, one rounding
 * per stored element.  blockIdx.y = column.  No reference counterpart. */
#include "hipk_internal.h"

template <typename T, int VW> struct alignas(sizeof(T) * VW) mg_pack { T v[VW]; };

/* grid position of flat point g, and the step to point g + 1 */
__device__ __forceinline__ void mg_coords(unsigned g, int n0, int n1, int &i0, int &i1, int &i2) {
   const unsigned r = g / (unsigned)n0;
   i0 = (int)(g - r * (unsigned)n0);
   i2 = (int)(r / (unsigned)n1);
   i1 = (int)(r - (unsigned)i2 * (unsigned)n1);
}
__device__ __forceinline__ void mg_next(int &i0, int &i1, int &i2, int n0, int n1) {
   if (++i0 == n0) { i0 = 0; if (++i1 == n1) { i1 = 0; ++i2; } }
}

/* sum_d w_d (2 c - lower - upper) at point g = (i0, i1, i2); the x neighbours are the caller's (registers or loads) */
template <typename T>
__device__ __forceinline__ double mg_laplacian(const T *__restrict__ yk, int64_t g, double c, double xl, double xr, int i1, int i2,
      int n0, int n1, int n2, int64_t plane, double w0, double w1, double w2) {
   double lap = 0.0;
   if (n0 > 1) lap = w0 * ((2.0 * c - xl) - xr);
   if (n1 > 1) {
      const double d = i1 > 0 ? (double)yk[g - n0] : 0.0, u = i1 < n1 - 1 ? (double)yk[g + n0] : 0.0;
      lap = fma(w1, (2.0 * c - d) - u, lap);
   }
   if (n2 > 1) {
      const double d = i2 > 0 ? (double)yk[g - plane] : 0.0, u = i2 < n2 - 1 ? (double)yk[g + plane] : 0.0;
      lap = fma(w2, (2.0 * c - d) - u, lap);
   }
   return lap;
}

template <typename T, int VW>
__global__ void __launch_bounds__(HIPK_BLOCK)
mg_step_kernel(int n0, int n1, int n2, double w0, double w1, double w2, hipk_cheb_coef cf, const T *X, int64_t ldx, const T *Yk,
      int64_t ldk, const T *Yp, int64_t ldp, T *Out, int64_t ldo) {
   typedef mg_pack<T, VW> P;
   const int c = blockIdx.y;
   const double cy = cf.cy[c], cp = cf.cp[c], cx = cf.cx[c], cw = cf.cw[c];
   const T *x = X + (size_t)c * ldx, *yk = Yk ? Yk + (size_t)c * ldk : NULL, *yp = Yp ? Yp + (size_t)c * ldp : NULL;
   T *out = Out + (size_t)c * ldo;
   const int64_t plane = (int64_t)n0 * n1, m = plane * n2, nv = m / VW;
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK, gid = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x;
   for (int64_t i = gid; i < nv; i += stride) {
      const int64_t g0 = i * VW;
      int i0, i1, i2;
      mg_coords((unsigned)g0, n0, n1, i0, i1, i2);
      const P px = ((const P *)x)[i];
      P pk = px, pp = px, po;
      if (yk) pk = ((const P *)yk)[i];
      if (yp) pp = ((const P *)yp)[i];
      /* the x neighbours outside the access: below its first point, above its last */
      const double below = (yk && i0 > 0) ? (double)yk[g0 - 1] : 0.0;
#pragma unroll
      for (int e = 0; e < VW; e++) {
         double s = cx * (double)px.v[e];
         if (yk) {
            const double cv = (double)pk.v[e];
            const double xl = e == 0 ? below : (i0 > 0 ? (double)pk.v[e > 0 ? e - 1 : 0] : 0.0);
            double xr = 0.0;
            if (i0 < n0 - 1) xr = e < VW - 1 ? (double)pk.v[e < VW - 1 ? e + 1 : e] : (double)yk[g0 + VW];
            const double lap = mg_laplacian<T>(yk, g0 + e, cv, xl, xr, i1, i2, n0, n1, n2, plane, w0, w1, w2);
            s = fma(cy, cv, s);
            if (yp) s = fma(cp, (double)pp.v[e], s);
            s = fma(cw, lap, s);
         } else if (yp) s = fma(cp, (double)pp.v[e], s);
         po.v[e] = (T)s;
         mg_next(i0, i1, i2, n0, n1);
      }
      ((P *)out)[i] = po;
   }
   /* the points past the last full access */
   for (int64_t g = nv * VW + gid; g < m; g += stride) {
      int i0, i1, i2;
      mg_coords((unsigned)g, n0, n1, i0, i1, i2);
      double s = cx * (double)x[g];
      if (yk) {
         const double cv = (double)yk[g];
         const double xl = i0 > 0 ? (double)yk[g - 1] : 0.0, xr = i0 < n0 - 1 ? (double)yk[g + 1] : 0.0;
         const double lap = mg_laplacian<T>(yk, g, cv, xl, xr, i1, i2, n0, n1, n2, plane, w0, w1, w2);
         s = fma(cy, cv, s);
         if (yp) s = fma(cp, (double)yp[g], s);
         s = fma(cw, lap, s);
      } else if (yp) s = fma(cp, (double)yp[g], s);
      out[g] = (T)s;
   }
}

/* coarse point (j0, j1, j2): sum over the fine points 2 j + 1 + {-1, 0, 1} of a coarsened dimension (weights 1/4, 1/2, 1/4; the
 * point 2 j + 2 may lie outside), the point j itself of a dimension that is kept; z outermost, x innermost */
template <typename T>
__device__ __forceinline__ double mg_restrict_point(const T *__restrict__ f, int j0, int j1, int j2, int nf0, int nf1, int nf2, int cz) {
   const int c0 = cz & 1, c1 = (cz >> 1) & 1, c2 = (cz >> 2) & 1;
   const int b0 = c0 ? 2 * j0 + 1 : j0, b1 = c1 ? 2 * j1 + 1 : j1, b2 = c2 ? 2 * j2 + 1 : j2;
   double s = 0.0;
   for (int d2 = -c2; d2 <= c2; d2++) {
      const int f2 = b2 + d2;
      if (f2 >= nf2) continue;
      const double wz = c2 ? (d2 ? 0.25 : 0.5) : 1.0;
      for (int d1 = -c1; d1 <= c1; d1++) {
         const int f1 = b1 + d1;
         if (f1 >= nf1) continue;
         const double wy = wz * (c1 ? (d1 ? 0.25 : 0.5) : 1.0);
         const T *row = f + ((int64_t)f2 * nf1 + f1) * nf0;
         for (int d0 = -c0; d0 <= c0; d0++) {
            const int f0 = b0 + d0;
            if (f0 >= nf0) continue;
            s = fma(wy * (c0 ? (d0 ? 0.25 : 0.5) : 1.0), (double)row[f0], s);
         }
      }
   }
   return s;
}

template <typename T, int VW>
__global__ void __launch_bounds__(HIPK_BLOCK)
mg_restrict_kernel(int nf0, int nf1, int nf2, int nc0, int nc1, int nc2, int cz, const T *F, int64_t ldf, T *C, int64_t ldc) {
   typedef mg_pack<T, VW> P;
   const T *f = F + (size_t)blockIdx.y * ldf;
   T *cc = C + (size_t)blockIdx.y * ldc;
   const int64_t m = (int64_t)nc0 * nc1 * nc2, nv = m / VW;
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK, gid = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x;
   for (int64_t i = gid; i < nv; i += stride) {
      int j0, j1, j2;
      mg_coords((unsigned)(i * VW), nc0, nc1, j0, j1, j2);
      P po;
#pragma unroll
      for (int e = 0; e < VW; e++) {
         po.v[e] = (T)mg_restrict_point<T>(f, j0, j1, j2, nf0, nf1, nf2, cz);
         mg_next(j0, j1, j2, nc0, nc1);
      }
      ((P *)cc)[i] = po;
   }
   for (int64_t g = nv * VW + gid; g < m; g += stride) {
      int j0, j1, j2;
      mg_coords((unsigned)g, nc0, nc1, j0, j1, j2);
      cc[g] = (T)mg_restrict_point<T>(f, j0, j1, j2, nf0, nf1, nf2, cz);
   }
}

/* the coarse points fine index i interpolates from along one dimension: a with weight wa, b with weight wb (0: none) */
__device__ __forceinline__ void mg_interp(int i, int nc, int coarsened, int &a, int &b, double &wa, double &wb) {
   if (!coarsened) { a = b = i; wa = 1.0; wb = 0.0; }
   else if (i & 1) { a = b = (i - 1) >> 1; wa = 1.0; wb = 0.0; }
   else {
      a = (i >> 1) - 1; b = i >> 1;
      wa = a >= 0 ? 0.5 : 0.0; wb = b < nc ? 0.5 : 0.0;
      if (a < 0) a = 0;
      if (b >= nc) b = nc - 1;
   }
}
/* y + (P c) at fine point (i0, i1, i2): at most 8 coarse points; a term of weight 0 is not read */
template <typename T>
__device__ __forceinline__ double mg_prolong_point(const T *__restrict__ cc, double y, int i0, int i1, int i2, int nc0, int nc1, int nc2, int cz) {
   int a[3][2];
   double w[3][2];
   mg_interp(i0, nc0, cz & 1, a[0][0], a[0][1], w[0][0], w[0][1]);
   mg_interp(i1, nc1, (cz >> 1) & 1, a[1][0], a[1][1], w[1][0], w[1][1]);
   mg_interp(i2, nc2, (cz >> 2) & 1, a[2][0], a[2][1], w[2][0], w[2][1]);
   double s = y;
#pragma unroll
   for (int q2 = 0; q2 < 2; q2++) {
      if (w[2][q2] == 0.0) continue;
#pragma unroll
      for (int q1 = 0; q1 < 2; q1++) {
         if (w[1][q1] == 0.0) continue;
         const T *row = cc + ((int64_t)a[2][q2] * nc1 + a[1][q1]) * nc0;
         const double wr = w[2][q2] * w[1][q1];
#pragma unroll
         for (int q0 = 0; q0 < 2; q0++)
            if (w[0][q0] != 0.0) s = fma(wr * w[0][q0], (double)row[a[0][q0]], s);
      }
   }
   return s;
}

template <typename T, int VW>
__global__ void __launch_bounds__(HIPK_BLOCK)
mg_prolong_kernel(int nf0, int nf1, int nf2, int nc0, int nc1, int nc2, int cz, const T *C, int64_t ldc, T *Y, int64_t ldy) {
   typedef mg_pack<T, VW> P;
   const T *cc = C + (size_t)blockIdx.y * ldc;
   T *y = Y + (size_t)blockIdx.y * ldy;
   const int64_t m = (int64_t)nf0 * nf1 * nf2, nv = m / VW;
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK, gid = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x;
   for (int64_t i = gid; i < nv; i += stride) {
      int i0, i1, i2;
      mg_coords((unsigned)(i * VW), nf0, nf1, i0, i1, i2);
      P py = ((const P *)y)[i];
#pragma unroll
      for (int e = 0; e < VW; e++) {
         py.v[e] = (T)mg_prolong_point<T>(cc, (double)py.v[e], i0, i1, i2, nc0, nc1, nc2, cz);
         mg_next(i0, i1, i2, nf0, nf1);
      }
      ((P *)y)[i] = py;
   }
   for (int64_t g = nv * VW + gid; g < m; g += stride) {
      int i0, i1, i2;
      mg_coords((unsigned)g, nf0, nf1, i0, i1, i2);
      y[g] = (T)mg_prolong_point<T>(cc, (double)y[g], i0, i1, i2, nc0, nc1, nc2, cz);
   }
}

/* ---- launchers ------------------------------------------------------------------------------------------------------- */
static int mg_num_cu(void) {
   static int num_cu = 0;                      /* launch geometry only: read the device once */
   if (num_cu == 0) {
      int dev = 0, n = 0;
      if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) num_cu = n;
      else num_cu = 256;
   }
   return num_cu;
}
static bool mg_al16(const void *p, int64_t ld, size_t es) { return !p || (((uintptr_t)p & 15) == 0 && ((size_t)ld * es) % 16 == 0); }
/* workgroups for m points, vw per lane and two trips per lane, at most eight per compute unit */
static unsigned mg_grid(int64_t m, int vw) {
   const int64_t per = (int64_t)HIPK_BLOCK * vw * 2, cap = (int64_t)mg_num_cu() * 8;
   int64_t gx = (m + per - 1) / per;
   if (gx > cap) gx = cap;
   return (unsigned)(gx < 1 ? 1 : gx);
}
/* the points of a grid, 0 when a length is below 1 or they pass INT32_MAX (the kernels divide in 32 bits) */
static int64_t mg_points(const int n[3]) {
   if (!n || n[0] < 1 || n[1] < 1 || n[2] < 1) return 0;
   const int64_t m = (int64_t)n[0] * n[1] * n[2];
   return ((int64_t)n[0] * n[1] > INT32_MAX || m > INT32_MAX) ? 0 : m;
}
/* bit d set: dimension d is coarsened; -1 when nc is not the coarse grid of nf */
static int mg_coarsened(const int nf[3], const int nc[3]) {
   int cz = 0;
   for (int d = 0; d < 3; d++) {
      if (nf[d] >= 3) {
         if (nc[d] != nf[d] / 2) return -1;
         cz |= 1 << d;
      } else if (nc[d] != nf[d]) return -1;
   }
   return cz;
}

extern "C" int hipk_mg_stencil_step(void *hip_stream, hipk_dtype dt, const int n[3], const double w[3], int nx, const hipk_cheb_coef *coef,
      const void *X, int64_t ldx, const void *Yk, int64_t ldk, const void *Yprev, int64_t ldp, void *Out, int64_t ldo) {
   if (dt != HIPK_F64 && dt != HIPK_F32) return -44;
   if (nx <= 0) return 0;
   const int64_t m = mg_points(n);
   if (m == 0 || !w || nx > HIPK_CHEB_MAXCOLS || !coef || !X || !Out || Out == Yk) return -1;
   hipStream_t st = (hipStream_t)hip_stream;
   hipk_prof_scope ps_(HIPK_PROF_VEC, st, hipk_stream_bytes(dt, m, (double)nx * (2 + (Yk != NULL) + (Yprev != NULL))));
   DISPATCH_RT(dt, {
      constexpr int VW = 16 / sizeof(T);
      const bool vec = mg_al16(X, ldx, sizeof(T)) && mg_al16(Yk, ldk, sizeof(T)) && mg_al16(Yprev, ldp, sizeof(T)) && mg_al16(Out, ldo, sizeof(T));
      const dim3 grid(mg_grid(m, vec ? VW : 1), nx);
      if (vec) hipLaunchKernelGGL((mg_step_kernel<T, VW>), grid, dim3(HIPK_BLOCK), 0, st, n[0], n[1], n[2], w[0], w[1], w[2], *coef, (const T *)X, ldx,
            (const T *)Yk, ldk, (const T *)Yprev, ldp, (T *)Out, ldo);
      else hipLaunchKernelGGL((mg_step_kernel<T, 1>), grid, dim3(HIPK_BLOCK), 0, st, n[0], n[1], n[2], w[0], w[1], w[2], *coef, (const T *)X, ldx,
            (const T *)Yk, ldk, (const T *)Yprev, ldp, (T *)Out, ldo);
   });
   HIPK_CHECK(hipGetLastError());
   return 0;
}

extern "C" int hipk_mg_restrict(void *hip_stream, hipk_dtype dt, const int nf[3], const int nc[3], int nx, const void *F, int64_t ldf,
      void *C, int64_t ldc) {
   if (dt != HIPK_F64 && dt != HIPK_F32) return -44;
   if (nx <= 0) return 0;
   const int64_t mf = mg_points(nf), mc = mg_points(nc);
   const int cz = mf && mc ? mg_coarsened(nf, nc) : -1;
   if (cz < 0 || nx > HIPK_CHEB_MAXCOLS || !F || !C || F == C) return -1;
   hipStream_t st = (hipStream_t)hip_stream;
   hipk_prof_scope ps_(HIPK_PROF_VEC, st, hipk_stream_bytes(dt, mf + mc, (double)nx));
   DISPATCH_RT(dt, {
      constexpr int VW = 16 / sizeof(T);
      const bool vec = mg_al16(C, ldc, sizeof(T));                 /* the stored panel; F is read point by point */
      const dim3 grid(mg_grid(mc, vec ? VW : 1), nx);
      if (vec) hipLaunchKernelGGL((mg_restrict_kernel<T, VW>), grid, dim3(HIPK_BLOCK), 0, st, nf[0], nf[1], nf[2], nc[0], nc[1], nc[2], cz,
            (const T *)F, ldf, (T *)C, ldc);
      else hipLaunchKernelGGL((mg_restrict_kernel<T, 1>), grid, dim3(HIPK_BLOCK), 0, st, nf[0], nf[1], nf[2], nc[0], nc[1], nc[2], cz,
            (const T *)F, ldf, (T *)C, ldc);
   });
   HIPK_CHECK(hipGetLastError());
   return 0;
}

extern "C" int hipk_mg_prolong_add(void *hip_stream, hipk_dtype dt, const int nf[3], const int nc[3], int nx, const void *C, int64_t ldc,
      void *Y, int64_t ldy) {
   if (dt != HIPK_F64 && dt != HIPK_F32) return -44;
   if (nx <= 0) return 0;
   const int64_t mf = mg_points(nf), mc = mg_points(nc);
   const int cz = mf && mc ? mg_coarsened(nf, nc) : -1;
   if (cz < 0 || nx > HIPK_CHEB_MAXCOLS || !C || !Y || C == Y) return -1;
   hipStream_t st = (hipStream_t)hip_stream;
   hipk_prof_scope ps_(HIPK_PROF_VEC, st, hipk_stream_bytes(dt, 2 * mf + mc, (double)nx));
   DISPATCH_RT(dt, {
      constexpr int VW = 16 / sizeof(T);
      const bool vec = mg_al16(Y, ldy, sizeof(T));                 /* the updated panel; C is read point by point */
      const dim3 grid(mg_grid(mf, vec ? VW : 1), nx);
      if (vec) hipLaunchKernelGGL((mg_prolong_kernel<T, VW>), grid, dim3(HIPK_BLOCK), 0, st, nf[0], nf[1], nf[2], nc[0], nc[1], nc[2], cz,
            (const T *)C, ldc, (T *)Y, ldy);
      else hipLaunchKernelGGL((mg_prolong_kernel<T, 1>), grid, dim3(HIPK_BLOCK), 0, st, nf[0], nf[1], nf[2], nc[0], nc[1], nc[2], cz,
            (const T *)C, ldc, (T *)Y, ldy);
   });
   HIPK_CHECK(hipGetLastError());
   return 0;
}
