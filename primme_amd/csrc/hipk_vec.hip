/* hipk_vec.hip — column utilities (scale, axpy, copy, gather, norms, pair products) and the fused vector passes of
 * the block QMR inner solver (gfx950): element-wise / few-array streaming kernels, one lane per row, two-stage
 * reductions with the library's fixed-order second stage.  UTIL_MAXCOLS, ColScal and ColPerm are in
 * hipk_panel_dev.h.
 */
#include "hipk_panel_dev.h"

/* Keeps the code of hipk_wave_sum what it is in the other units.  __shfl_down of the HIP headers is a plain inline
 * function with the width as an argument; every call in this unit passes 64, and when no other width is in sight the
 * compiler propagates the constant into the function before it inlines it, after which the lane-index clamp of the
 * five shuffle steps is formed differently (lane & 63 against 64 - off becomes ~lane & 63 against off: one VALU
 * instruction more in the set-up of every two-stage reduction kernel below).  hipk_panels.hip and hipk_ritz.hip hold
 * calls with widths 8 / 16 / 32 (ritz_big_kernel, hipk_inkernel_finalize); this one retained call does the same
 * here.  It is no kernel and nothing calls it; scripts/device_digest.py shows the effect of removing it. */
__attribute__((used)) __device__ double vec_shfl_width_anchor(double v) { return __shfl_down(v, 8, 16); }

/* ============================ column utilities ================================ */
template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
scale_kernel(T *__restrict__ X, int64_t ldX, int nx, ColScal sc, int64_t m) {
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int c = 0; c < nx; c++) {
      T *x = X + (size_t)c * ldX;
      const double a = sc.a[c];
      for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride)
         x[i] = (T)(a * (double)x[i]);
   }
}

template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
scale_rsqrt_kernel(T *__restrict__ X, int64_t ldX, int nx, const double *__restrict__ norm2, int64_t m) {
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int c = 0; c < nx; c++) {
      T *x = X + (size_t)c * ldX;
      const double a = 1.0 / sqrt(norm2[c]);     /* same two IEEE operations as the host path */
      for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride)
         x[i] = (T)(a * (double)x[i]);
   }
}

/* Y = i * X for columns holding (re, im) pairs: (re, im) -> (-im, re).  One pair per lane
 * visit, 16- or 8-byte accesses. */
template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
pair_rotate_kernel(const T *__restrict__ X, int64_t ldX, T *__restrict__ Y, int64_t ldY, int nx, int64_t npairs) {
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int c = 0; c < nx; c++) {
      const T *x = X + (size_t)c * ldX;
      T *y = Y + (size_t)c * ldY;
      for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < npairs; i += stride) {
         const T re = x[2 * i], im = x[2 * i + 1];
         y[2 * i] = -im;
         y[2 * i + 1] = re;
      }
   }
}

template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
axpy_kernel(ColScal sc, const T *__restrict__ X, int64_t ldX, T *__restrict__ Y, int64_t ldY,
      int nx, int64_t m) {
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int c = 0; c < nx; c++) {
      const T *x = X + (size_t)c * ldX;
      T *y = Y + (size_t)c * ldY;
      const double a = sc.a[c];
      for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride)
         y[i] = (T)fma(a, (double)x[i], (double)y[i]);
   }
}

template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
xpay_kernel(ColScal sc, const T *__restrict__ X, int64_t ldX, T *__restrict__ Y, int64_t ldY,
      int nx, int64_t m) {
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int c = 0; c < nx; c++) {
      const T *x = X + (size_t)c * ldX;
      T *y = Y + (size_t)c * ldY;
      const double a = sc.a[c];
      for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride)
         y[i] = (T)fma(a, (double)y[i], (double)x[i]);
   }
}

template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
gather_kernel(const T *__restrict__ X, int64_t ldX, ColPerm pm, int n, T *__restrict__ Y,
      int64_t ldY, int64_t m) {
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int c = 0; c < n; c++) {
      const T *x = X + (size_t)pm.p[c] * ldX;
      T *y = Y + (size_t)c * ldY;
      for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride)
         y[i] = x[i];
   }
}

template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
norms2_kernel(const T *__restrict__ X, int64_t ldX, int nx, int64_t m,
      double *__restrict__ partials) {
   __shared__ double sm[HIPK_BLOCK / HIPK_WAVE];
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int c = 0; c < nx; c++) {
      const T *x = X + (size_t)c * ldX;
      double s = 0.0;
      for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride) {
         double v = (double)x[i];
         s = fma(v, v, s);
      }
      s = hipk_wave_sum(s);
      if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
      __syncthreads();
      if (threadIdx.x == 0) partials[(size_t)blockIdx.x * nx + c] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
      __syncthreads();
   }
}

template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
residual_kernel(const T *__restrict__ X, int64_t ldX, T *__restrict__ Wr, int64_t ldW, int nx,
      ColScal th, int64_t m, double *__restrict__ partials) {
   __shared__ double sm[HIPK_BLOCK / HIPK_WAVE];
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int c = 0; c < nx; c++) {
      const T *x = X + (size_t)c * ldX;
      T *w = Wr + (size_t)c * ldW;
      const double t = th.a[c];
      double s = 0.0;
      for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride) {
         T r = (T)fma(-t, (double)x[i], (double)w[i]);
         w[i] = r;
         s = fma((double)r, (double)r, s);
      }
      s = hipk_wave_sum(s);
      if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
      __syncthreads();
      if (threadIdx.x == 0) partials[(size_t)blockIdx.x * nx + c] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
      __syncthreads();
   }
}

/* out[c] = X(:,c)' Y(:,c): b independent dot products (block QMR recurrences) */
template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
pair_dots_kernel(const T *__restrict__ X, int64_t ldX, const T *__restrict__ Y, int64_t ldY, int nx,
      int64_t m, double *__restrict__ partials) {
   __shared__ double sm[HIPK_BLOCK / HIPK_WAVE];
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int c = 0; c < nx; c++) {
      const T *x = X + (size_t)c * ldX;
      const T *y = Y + (size_t)c * ldY;
      double s = 0.0;
      for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride)
         s = fma((double)x[i], (double)y[i], s);
      s = hipk_wave_sum(s);
      if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
      __syncthreads();
      if (threadIdx.x == 0) partials[(size_t)blockIdx.x * nx + c] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
      __syncthreads();
   }
}

/* y += a x (stored); out[c] = z'y or y'y: the axpy and the dot that follows it in one pass */
template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
axpy_dot_kernel(ColScal sc, const T *__restrict__ X, int64_t ldX, T *__restrict__ Y, int64_t ldY,
      const T *__restrict__ Z, int64_t ldZ, int nx, int64_t m, double *__restrict__ partials) {
   __shared__ double sm[HIPK_BLOCK / HIPK_WAVE];
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int c = 0; c < nx; c++) {
      const T *x = X + (size_t)c * ldX;
      T *y = Y + (size_t)c * ldY;
      const T *z = Z ? Z + (size_t)c * ldZ : NULL;
      const double a = sc.a[c];
      double s = 0.0;
      for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride) {
         const T ny = (T)fma(a, (double)x[i], (double)y[i]);
         y[i] = ny;
         s = fma(z ? (double)z[i] : (double)ny, (double)ny, s);
      }
      s = hipk_wave_sum(s);
      if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
      __syncthreads();
      if (threadIdx.x == 0) partials[(size_t)blockIdx.x * nx + c] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
      __syncthreads();
   }
}

/* delta = gamma*delta + eta*d; sol += delta; out[c] = |sol(:,c)|^2  (one pass, block QMR) */
template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
qmr_update_kernel(ColScal gam, ColScal eta, const T *__restrict__ D, int64_t ldD, T *__restrict__ Delta,
      int64_t ldDelta, T *__restrict__ Sol, int64_t ldSol, int nx, int64_t m, double *__restrict__ partials) {
   __shared__ double sm[HIPK_BLOCK / HIPK_WAVE];
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int c = 0; c < nx; c++) {
      const T *d = D + (size_t)c * ldD;
      T *de = Delta + (size_t)c * ldDelta;
      T *so = Sol + (size_t)c * ldSol;
      const double g = gam.a[c], e = eta.a[c];
      double s = 0.0;
      for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride) {
         T nd = (T)fma((double)de[i], g, (double)d[i] * e);
         de[i] = nd;
         T ns = (T)((double)nd + (double)so[i]);
         so[i] = ns;
         s = fma((double)ns, (double)ns, s);
      }
      s = hipk_wave_sum(s);
      if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
      __syncthreads();
      if (threadIdx.x == 0) partials[(size_t)blockIdx.x * nx + c] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
      __syncthreads();
   }
}

/* The QMR step and the next application of the Jacobi preconditioner in one pass (block QMR):
 *    delta = gamma delta + eta d;  sol += delta;  out[c] = |sol(:,c)|^2
 *    w = g ./ (diag - shift[c]);                  out[nx + c] = g(:,c)' w(:,c)
 * Three launches of the unfused sequence (qmr_update, jacobi, pair_dots) read g twice and w once more
 * than this does (reference inner_solve.c:384-397 fuses the first line on the CPU; :619-634 is the second). */
template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
qmr_update_jacobi_kernel(ColScal gam, ColScal eta, ColScal shf, double min_den, const T *__restrict__ D, int64_t ldD,
      T *__restrict__ Delta, int64_t ldDelta, T *__restrict__ Sol, int64_t ldSol, const T *__restrict__ G, int64_t ldG,
      const T *__restrict__ diag, T *__restrict__ Wp, int64_t ldW, int nx, int c0, int64_t m, double *__restrict__ partials) {
   /* rows outside, (up to 8) columns inside: the diagonal is read once per row, not once per column */
   constexpr int NXC = 8;
   __shared__ double sm[HIPK_BLOCK / HIPK_WAVE][2 * NXC];
   const int nc = min(NXC, nx - c0);
   double s1[NXC], s2[NXC];
#pragma unroll
   for (int c = 0; c < NXC; c++) { s1[c] = 0.0; s2[c] = 0.0; }
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride) {
      const double dg = (double)diag[i];
#pragma unroll
      for (int c = 0; c < NXC; c++)
         if (c < nc) {
            const size_t cc = (size_t)(c0 + c);
            const T nd = (T)fma((double)Delta[i + cc * ldDelta], gam.a[c0 + c], (double)D[i + cc * ldD] * eta.a[c0 + c]);
            Delta[i + cc * ldDelta] = nd;
            const T ns = (T)((double)nd + (double)Sol[i + cc * ldSol]);
            Sol[i + cc * ldSol] = ns;
            s1[c] = fma((double)ns, (double)ns, s1[c]);
            double den = dg - shf.a[c0 + c];
            if (fabs(den) <= min_den) den = copysign(min_den, den);       /* a NaN stays a NaN */
            const double gi = (double)G[i + cc * ldG];
            const T wi = (T)(gi / den);
            Wp[i + cc * ldW] = wi;
            s2[c] = fma(gi, (double)wi, s2[c]);
         }
   }
   const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
   for (int c = 0; c < NXC; c++) {
      const double a = hipk_wave_sum(s1[c]), b = hipk_wave_sum(s2[c]);
      if (lane == 0) { sm[wv][c] = a; sm[wv][NXC + c] = b; }
   }
   __syncthreads();
   if (threadIdx.x < 2 * NXC) {
      const int which = threadIdx.x / NXC, c = threadIdx.x % NXC;
      if (c < nc)
         partials[(size_t)blockIdx.x * 2 * nx + which * nx + c0 + c] =
               (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
   }
}

/* out[c] = x_c' w_c, out[nx + c] = v_c' w_c, out[2 nx + c] = v_c' x_c in one pass over the three panels: what
 * the block QMR step needs to form sigma = v'(I - x x')w = v'w - (x'w)(v'x) without first storing the projected w */
template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
triple_dots_kernel(const T *__restrict__ X, int64_t ldX, const T *__restrict__ Vv, int64_t ldV, const T *__restrict__ Wv,
      int64_t ldW, int nx, int64_t m, double *__restrict__ partials) {
   __shared__ double sm[HIPK_BLOCK / HIPK_WAVE][3];
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int c = 0; c < nx; c++) {
      const T *x = X + (size_t)c * ldX, *v = Vv + (size_t)c * ldV, *w = Wv + (size_t)c * ldW;
      double a = 0.0, b = 0.0, d = 0.0;
      for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride) {
         const double xi = (double)x[i], vi = (double)v[i], wi = (double)w[i];
         a = fma(xi, wi, a); b = fma(vi, wi, b); d = fma(vi, xi, d);
      }
      a = hipk_wave_sum(a); b = hipk_wave_sum(b); d = hipk_wave_sum(d);
      if ((threadIdx.x & 63) == 0) { sm[threadIdx.x >> 6][0] = a; sm[threadIdx.x >> 6][1] = b; sm[threadIdx.x >> 6][2] = d; }
      __syncthreads();
      if (threadIdx.x < 3)
         partials[(size_t)blockIdx.x * 3 * nx + threadIdx.x * nx + c] =
               (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
      __syncthreads();
   }
}

/* g_c -= alpha_c (w_c - xr_c x_c), out[c] = g_c' g_c: the projection of w against x and the residual update of
 * the QMR step in one pass; the projected w itself is never stored (inner_solve.c:853-880, :371-377) */
template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
axpy_proj_dot_kernel(ColScal alpha, ColScal xr, const T *__restrict__ Wv, int64_t ldW, const T *__restrict__ X, int64_t ldX,
      T *__restrict__ G, int64_t ldG, int nx, int64_t m, double *__restrict__ partials) {
   __shared__ double sm[HIPK_BLOCK / HIPK_WAVE];
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int c = 0; c < nx; c++) {
      const T *w = Wv + (size_t)c * ldW, *x = X + (size_t)c * ldX;
      T *g = G + (size_t)c * ldG;
      const double a = alpha.a[c], r = xr.a[c];
      double s = 0.0;
      for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride) {
         const T wp = (T)fma(-r, (double)x[i], (double)w[i]);          /* rounded like the stored projected w */
         const T ng = (T)fma(-a, (double)wp, (double)g[i]);
         g[i] = ng;
         s = fma((double)ng, (double)ng, s);
      }
      s = hipk_wave_sum(s);
      if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
      __syncthreads();
      if (threadIdx.x == 0) partials[(size_t)blockIdx.x * nx + c] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
      __syncthreads();
   }
}

/* The same with the NEXT inner product of the preconditioned QMR already taken: out[nx + c] = g_c' K^-1 g_c for the
 * updated g and the Jacobi preconditioner K = diag - shift[c].  With rho known at this synchronisation the step's
 * beta = rho / rho_prev is known before the QMR update runs, and that pass can write the new direction
 * d = K^-1 g + beta d in place (qmr_update_dir_kernel) instead of storing w = K^-1 g and adding beta d in a further pass.
 * Rows outside, (up to 8) columns inside: the diagonal is read once per row. */
/* ---- the scalar recurrences of one block-QMR step, evaluated ON THE DEVICE (eigs_jd.c: the step with one host synchronisation).
 * The launches that apply a step's coefficients compute them in their prologue, every lane for itself, from the reduction
 * results of the launches before them — still in HBM — and from the previous step's state, passed by value.  The host evaluates
 * the same expressions on the mirrored results after its one wait; both sides round every operation separately (no
 * contraction here, ISO C on the host), division and square root are correctly rounded on both: the same bits.
 *   tri = [x'w | v'w | v'x] (hipk_triple_dots), ggr = [g'g | g'K^-1 g] (hipk_axpy_proj_dot_jacobi_dev) */
struct QmrPrev { double rho_prev[8], tau_prev[8], theta_prev[8]; double eps; };
__device__ __forceinline__ void qmr_alpha_dev(const double *__restrict__ tri, int nx, int col, double rho_prev, double eps, double &alpha, double &xr) {
#pragma clang fp contract(off)
   xr = tri[col];
   const double t = xr * tri[2 * nx + col];
   const double sigma = tri[nx + col] - t;
   bool bad = !isfinite(sigma) || sigma == 0.0;
   double a = 0.0;
   if (!bad) {
      a = rho_prev / sigma;
      bad = !isfinite(a) || fabs(a) < eps || fabs(a) > 1.0 / eps;
   }
   alpha = bad ? 0.0 : a;                        /* 0: the column leaves the block at this step (the host sees the same) */
}
__device__ __forceinline__ void qmr_coeffs_dev(const double *__restrict__ ggr, int nx, int col, double alpha, double rho_prev, double tau_prev,
      double theta_prev, double &gam, double &eta, double &bet) {
#pragma clang fp contract(off)
   const double theta = sqrt(ggr[col]) / tau_prev;
   const double t2 = theta * theta;
   const double c = 1.0 / sqrt(1 + t2);
   const double cc = c * c;
   const double g1 = cc * theta_prev;
   gam = g1 * theta_prev;
   const double e1 = alpha * c;
   eta = e1 * c;
   bet = ggr[nx + col] / rho_prev;
}

template <typename T, bool DEV>
__global__ void __launch_bounds__(HIPK_BLOCK)
axpy_proj_dot_jacobi_kernel(ColScal alpha, ColScal xr, ColScal shf, double min_den, const T *__restrict__ Wv, int64_t ldW,
      const T *__restrict__ X, int64_t ldX, T *__restrict__ G, int64_t ldG, const T *__restrict__ diag, int nx, int c0, int64_t m,
      double *__restrict__ partials, const double *__restrict__ tri, QmrPrev pv) {
   constexpr int NXC = 8;
   __shared__ double sm[HIPK_BLOCK / HIPK_WAVE][2 * NXC];
   const int nc = min(NXC, nx - c0);
   double s1[NXC], s2[NXC], al[NXC], xq[NXC];
#pragma unroll
   for (int c = 0; c < NXC; c++) {
      s1[c] = 0.0; s2[c] = 0.0; al[c] = 0.0; xq[c] = 0.0;
      if (c < nc) {
         if (DEV) qmr_alpha_dev(tri, nx, c0 + c, pv.rho_prev[c], pv.eps, al[c], xq[c]);
         else { al[c] = alpha.a[c0 + c]; xq[c] = xr.a[c0 + c]; }
      }
   }
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride) {
      const double dg = (double)diag[i];
#pragma unroll
      for (int c = 0; c < NXC; c++)
         if (c < nc) {
            const size_t cc = (size_t)(c0 + c);
            const T wp = (T)fma(-xq[c], (double)X[i + cc * ldX], (double)Wv[i + cc * ldW]);   /* rounded like the stored projected w */
            const T ng = (T)fma(-al[c], (double)wp, (double)G[i + cc * ldG]);
            G[i + cc * ldG] = ng;
            s1[c] = fma((double)ng, (double)ng, s1[c]);
            double den = dg - shf.a[c0 + c];
            if (fabs(den) <= min_den) den = copysign(min_den, den);       /* a NaN stays a NaN */
            const T wi = (T)((double)ng / den);                      /* rounded like the stored K^-1 g */
            s2[c] = fma((double)ng, (double)wi, s2[c]);
         }
   }
   const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
   for (int c = 0; c < NXC; c++) {
      const double a = hipk_wave_sum(s1[c]), b = hipk_wave_sum(s2[c]);
      if (lane == 0) { sm[wv][c] = a; sm[wv][NXC + c] = b; }
   }
   __syncthreads();
   if (threadIdx.x < 2 * NXC) {
      const int which = threadIdx.x / NXC, c = threadIdx.x % NXC;
      if (c < nc)
         partials[(size_t)blockIdx.x * 2 * nx + which * nx + c0 + c] =
               (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
   }
}

/* delta = gamma delta + eta d;  sol += delta;  out[c] = |sol(:,c)|^2;  d = g ./ (diag - shift[c]) + beta d (in place):
 * the QMR step and the next search direction in one pass over d, delta, sol, g (seven array passes per column; the
 * sequence qmr_update_jacobi + axpy it replaces makes eleven) */
template <typename T, bool DEV>
__global__ void __launch_bounds__(HIPK_BLOCK)
qmr_update_dir_kernel(ColScal gam, ColScal eta, ColScal bet, ColScal shf, double min_den, T *__restrict__ D, int64_t ldD,
      T *__restrict__ Delta, int64_t ldDelta, T *__restrict__ Sol, int64_t ldSol, const T *__restrict__ G, int64_t ldG,
      const T *__restrict__ diag, int nx, int c0, int64_t m, double *__restrict__ partials, const double *__restrict__ tri,
      const double *__restrict__ ggr, QmrPrev pv) {
   constexpr int NXC = 8;
   __shared__ double sm[HIPK_BLOCK / HIPK_WAVE][NXC];
   const int nc = min(NXC, nx - c0);
   double s1[NXC], ga[NXC], et[NXC], be[NXC];
   bool live[NXC];                  /* DEV: a column whose alpha was unusable leaves the block before this update (its sol stays) */
#pragma unroll
   for (int c = 0; c < NXC; c++) {
      s1[c] = 0.0; ga[c] = 0.0; et[c] = 0.0; be[c] = 0.0; live[c] = c < nc;
      if (c < nc) {
         if (DEV) {
            double a, x_;
            qmr_alpha_dev(tri, nx, c0 + c, pv.rho_prev[c], pv.eps, a, x_);
            live[c] = a != 0.0;
            if (live[c]) qmr_coeffs_dev(ggr, nx, c0 + c, a, pv.rho_prev[c], pv.tau_prev[c], pv.theta_prev[c], ga[c], et[c], be[c]);
         } else { ga[c] = gam.a[c0 + c]; et[c] = eta.a[c0 + c]; be[c] = bet.a[c0 + c]; }
      }
   }
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride) {
      const double dg = (double)diag[i];
#pragma unroll
      for (int c = 0; c < NXC; c++)
         if (live[c]) {
            const size_t cc = (size_t)(c0 + c);
            const double di = (double)D[i + cc * ldD];
            const T nd = (T)fma((double)Delta[i + cc * ldDelta], ga[c], di * et[c]);
            Delta[i + cc * ldDelta] = nd;
            const T ns = (T)((double)nd + (double)Sol[i + cc * ldSol]);
            Sol[i + cc * ldSol] = ns;
            s1[c] = fma((double)ns, (double)ns, s1[c]);
            double den = dg - shf.a[c0 + c];
            if (fabs(den) <= min_den) den = copysign(min_den, den);       /* a NaN stays a NaN */
            const T wi = (T)((double)G[i + cc * ldG] / den);
            D[i + cc * ldD] = (T)fma(be[c], di, (double)wi);    /* w += beta d, as the axpy pass rounds it */
         }
   }
   const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
   for (int c = 0; c < NXC; c++) {
      const double a = hipk_wave_sum(s1[c]);
      if (lane == 0) sm[wv][c] = a;
   }
   __syncthreads();
   if (threadIdx.x < NXC && (int)threadIdx.x < nc)
      partials[(size_t)blockIdx.x * nx + c0 + threadIdx.x] = (sm[0][threadIdx.x] + sm[1][threadIdx.x]) + (sm[2][threadIdx.x] + sm[3][threadIdx.x]);
}

/* A pass with a two-stage reduction: launch(gx) enqueues the kernels that leave nout partial sums per workgroup in
 * ctx->partials (gx workgroups: every reduction here uses the same grid, so fused and unfused passes give the same
 * sums), the second stage adds them into out_dev. */
template <typename F>
static int reduce_pass(hipk_ctx *ctx, int64_t m, int nout, double *out_dev, F launch) {
   const int gx = hipk_grid_for_rows(ctx, m, HIPK_BLOCK * 4, 4);
   if (hipk_reserve_partials(ctx, (size_t)gx * nout)) return -2;
   const int rc = launch(gx);
   if (rc) return rc;
   HIPK_CHECK(hipGetLastError());
   return hipk_finalize_partials(ctx, ctx->partials, gx, nout, out_dev);
}

extern "C" int hipk_scale_cols(hipk_ctx *ctx, hipk_dtype dt, int64_t m, void *X, int64_t ldX,
      int nx, const double *alpha_host) {
   /* real factors on complex columns: the real kernel on the panel seen as 2m reals */
   if (HIPK_IS_Z(dt)) return hipk_scale_cols(ctx, hipk_real_of(dt), 2 * m, X, 2 * ldX, nx, alpha_host);
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(2 * nx)));
   const int gx = hipk_grid_for_rows(ctx, m, HIPK_BLOCK * 4, 8);
   for (int c0 = 0; c0 < nx; c0 += UTIL_MAXCOLS) {
      const int n = nx - c0 < UTIL_MAXCOLS ? nx - c0 : UTIL_MAXCOLS;
      ColScal sc;
      for (int c = 0; c < n; c++) sc.a[c] = alpha_host[c0 + c];
      DISPATCH_RT(dt, hipLaunchKernelGGL(scale_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, (T *)X + (size_t)c0 * ldX, ldX, n, sc, m));
      HIPK_CHECK(hipGetLastError());
   }
   return 0;
}

extern "C" int hipk_scale_cols_rsqrt_dev(hipk_ctx *ctx, hipk_dtype dt, int64_t m, void *X, int64_t ldX,
      int nx, const double *norm2_dev) {
   if (nx <= 0) return 0;
   if (HIPK_IS_Z(dt)) return hipk_scale_cols_rsqrt_dev(ctx, hipk_real_of(dt), 2 * m, X, 2 * ldX, nx, norm2_dev);
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(2 * nx)));
   int gx = hipk_grid_for_rows(ctx, m, HIPK_BLOCK * 4, 8);
   DISPATCH_RT(dt, hipLaunchKernelGGL(scale_rsqrt_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, (T *)X, ldX, nx, norm2_dev, m));
   HIPK_CHECK(hipGetLastError());
   return 0;
}

extern "C" int hipk_axpy_cols(hipk_ctx *ctx, hipk_dtype dt, int64_t m, const double *alpha_host,
      const void *X, int64_t ldX, void *Y, int64_t ldY, int nx) {
   if (HIPK_IS_Z(dt)) return hipk_z_axpy(ctx, dt, m, alpha_host, X, ldX, Y, ldY, nx, 0);      /* (re, im) factors */
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(3 * nx)));
   const int gx = hipk_grid_for_rows(ctx, m, HIPK_BLOCK * 4, 8);
   for (int c0 = 0; c0 < nx; c0 += UTIL_MAXCOLS) {
      const int n = nx - c0 < UTIL_MAXCOLS ? nx - c0 : UTIL_MAXCOLS;
      ColScal sc;
      for (int c = 0; c < n; c++) sc.a[c] = alpha_host[c0 + c];
      DISPATCH_RT(dt, hipLaunchKernelGGL(axpy_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, sc, (const T *)X + (size_t)c0 * ldX, ldX, (T *)Y + (size_t)c0 * ldY, ldY, n, m));
      HIPK_CHECK(hipGetLastError());
   }
   return 0;
}

extern "C" int hipk_pair_rotate(hipk_ctx *ctx, hipk_dtype dt, int64_t npairs, const void *X, int64_t ldX,
      void *Y, int64_t ldY, int nx) {
   if (nx <= 0 || npairs <= 0) return 0;
   int gx = hipk_grid_for_rows(ctx, npairs, HIPK_BLOCK * 4, 8);
   DISPATCH_RT(dt, hipLaunchKernelGGL(pair_rotate_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, (const T *)X, ldX, (T *)Y, ldY, nx, npairs));
   HIPK_CHECK(hipGetLastError());
   return 0;
}

/* column copy: 16 bytes per lane when the columns allow it (the runtime's 2-D copy reaches 2.4 TB/s) */
template <typename U>
__global__ void __launch_bounds__(HIPK_BLOCK)
copy_cols_kernel(const char *__restrict__ X, size_t ldx_bytes, char *__restrict__ Y, size_t ldy_bytes, size_t n) {
   const U *x = (const U *)(X + (size_t)blockIdx.y * ldx_bytes);
   U *y = (U *)(Y + (size_t)blockIdx.y * ldy_bytes);
   const size_t stride = (size_t)gridDim.x * HIPK_BLOCK;
   size_t i = (size_t)blockIdx.x * HIPK_BLOCK + threadIdx.x;
   for (; i + 3 * stride < n; i += 4 * stride) {
      const U a = x[i], b = x[i + stride], c = x[i + 2 * stride], d = x[i + 3 * stride];
      y[i] = a; y[i + stride] = b; y[i + 2 * stride] = c; y[i + 3 * stride] = d;
   }
   for (; i < n; i += stride) y[i] = x[i];
}

extern "C" int hipk_copy_cols(hipk_ctx *ctx, hipk_dtype dt, int64_t m, const void *X,
      int64_t ldX, void *Y, int64_t ldY, int nx) {
   const size_t es = hipk_elem_size(dt);
   if (nx <= 0 || m <= 0) return 0;
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(2 * nx)));
   const size_t bytes = (size_t)m * es, lx = (size_t)ldX * es, ly = (size_t)ldY * es;
   if (nx > 65535 || bytes < 4096) {
      HIPK_CHECK(hipMemcpy2DAsync(Y, ly, X, lx, bytes, (size_t)nx, hipMemcpyDeviceToDevice, ctx->stream));
      return 0;
   }
   const bool v16 = ((uintptr_t)X % 16 == 0) && ((uintptr_t)Y % 16 == 0) && (nx == 1 || (lx % 16 == 0 && ly % 16 == 0));
   const size_t us = v16 ? 16 : (es == 4 ? 4 : 8);             /* bytes per lane visit */
   const size_t n = bytes / us, head = n * us;
   int gx = hipk_grid_for_rows(ctx, (int64_t)n, HIPK_BLOCK * 4, 8);
   if (nx > 1) { gx = (gx + nx - 1) / nx; if (gx < 1) gx = 1; }
   dim3 grid(gx, nx);
   if (v16) hipLaunchKernelGGL(copy_cols_kernel<uint4>, grid, dim3(HIPK_BLOCK), 0, ctx->stream, (const char *)X, lx, (char *)Y, ly, n);
   else if (es == 4) hipLaunchKernelGGL(copy_cols_kernel<unsigned int>, grid, dim3(HIPK_BLOCK), 0, ctx->stream, (const char *)X, lx, (char *)Y, ly, n);
   else hipLaunchKernelGGL(copy_cols_kernel<unsigned long long>, grid, dim3(HIPK_BLOCK), 0, ctx->stream, (const char *)X, lx, (char *)Y, ly, n);
   HIPK_CHECK(hipGetLastError());
   if (head < bytes)    /* fewer than 16 bytes per column left over */
      HIPK_CHECK(hipMemcpy2DAsync((char *)Y + head, ly, (const char *)X + head, lx, bytes - head, (size_t)nx, hipMemcpyDeviceToDevice, ctx->stream));
   return 0;
}

extern "C" int hipk_gather_cols(hipk_ctx *ctx, hipk_dtype dt, int64_t m, const void *X,
      int64_t ldX, const int *perm_host, int n, void *Y, int64_t ldY) {
   if (HIPK_IS_Z(dt)) return hipk_gather_cols(ctx, hipk_real_of(dt), 2 * m, X, 2 * ldX, perm_host, n, Y, 2 * ldY);
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(2 * n)));
   const int gx = hipk_grid_for_rows(ctx, m, HIPK_BLOCK * 4, 8);
   for (int c0 = 0; c0 < n; c0 += UTIL_MAXCOLS) {
      const int nn = n - c0 < UTIL_MAXCOLS ? n - c0 : UTIL_MAXCOLS;
      ColPerm pm;
      for (int c = 0; c < nn; c++) pm.p[c] = perm_host[c0 + c];
      DISPATCH_RT(dt, hipLaunchKernelGGL(gather_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, (const T *)X, ldX, pm, nn, (T *)Y + (size_t)c0 * ldY, ldY, m));
      HIPK_CHECK(hipGetLastError());
   }
   return 0;
}

extern "C" int hipk_col_norms2(hipk_ctx *ctx, hipk_dtype dt, int64_t m, const void *X,
      int64_t ldX, int nx, double *out_dev) {
   if (nx <= 0) return 0;
   if (HIPK_IS_Z(dt)) return hipk_col_norms2(ctx, hipk_real_of(dt), 2 * m, X, 2 * ldX, nx, out_dev);   /* |z|^2 = re^2 + im^2 */
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(nx)));
   return reduce_pass(ctx, m, nx, out_dev, [&](int gx) -> int {
      DISPATCH_RT(dt, hipLaunchKernelGGL(norms2_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, (const T *)X, ldX, nx, m, ctx->partials));
      return 0;
   });
}

extern "C" int hipk_residual_cols(hipk_ctx *ctx, hipk_dtype dt, int64_t m, const void *X,
      int64_t ldX, void *Wr, int64_t ldW, int nx, const double *theta_host, double *nrm2_dev) {
   if (HIPK_IS_Z(dt)) return hipk_residual_cols(ctx, hipk_real_of(dt), 2 * m, X, 2 * ldX, Wr, 2 * ldW, nx, theta_host, nrm2_dev);   /* theta is real */
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(3 * nx)));
   const size_t es = hipk_elem_size(dt);
   for (int c0 = 0; c0 < nx; c0 += UTIL_MAXCOLS) {
      const int n = nx - c0 < UTIL_MAXCOLS ? nx - c0 : UTIL_MAXCOLS;
      ColScal th;
      for (int c = 0; c < n; c++) th.a[c] = theta_host[c0 + c];
      const char *Xc = (const char *)X + (size_t)c0 * ldX * es;
      char *Wc = (char *)Wr + (size_t)c0 * ldW * es;
      const int rc = reduce_pass(ctx, m, n, nrm2_dev + c0, [&](int gx) -> int {
         DISPATCH_RT(dt, hipLaunchKernelGGL(residual_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, (const T *)Xc, ldX, (T *)Wc, ldW, n, th, m, ctx->partials));
         return 0;
      });
      if (rc) return rc;
   }
   return 0;
}

extern "C" int hipk_pair_dots(hipk_ctx *ctx, hipk_dtype dt, int64_t m, const void *X, int64_t ldX,
      const void *Y, int64_t ldY, int nx, double *out_dev) {
   if (nx <= 0) return 0;
   if (HIPK_IS_Z(dt)) return hipk_z_pair_dots(ctx, dt, m, X, ldX, Y, ldY, nx, out_dev);
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(2 * nx)));
   return reduce_pass(ctx, m, nx, out_dev, [&](int gx) -> int {
      DISPATCH_RT(dt, hipLaunchKernelGGL(pair_dots_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, (const T *)X, ldX, (const T *)Y, ldY, nx, m, ctx->partials));
      return 0;
   });
}

extern "C" int hipk_xpay_cols(hipk_ctx *ctx, hipk_dtype dt, int64_t m, const double *alpha_host,
      const void *X, int64_t ldX, void *Y, int64_t ldY, int nx) {
   if (HIPK_IS_Z(dt)) return hipk_z_axpy(ctx, dt, m, alpha_host, X, ldX, Y, ldY, nx, 1);
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(3 * nx)));
   const int gx = hipk_grid_for_rows(ctx, m, HIPK_BLOCK * 4, 8);
   for (int c0 = 0; c0 < nx; c0 += UTIL_MAXCOLS) {
      const int n = nx - c0 < UTIL_MAXCOLS ? nx - c0 : UTIL_MAXCOLS;
      ColScal sc;
      for (int c = 0; c < n; c++) sc.a[c] = alpha_host[c0 + c];
      DISPATCH_RT(dt, hipLaunchKernelGGL(xpay_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, sc, (const T *)X + (size_t)c0 * ldX, ldX, (T *)Y + (size_t)c0 * ldY, ldY, n, m));
      HIPK_CHECK(hipGetLastError());
   }
   return 0;
}

extern "C" int hipk_axpy_dot(hipk_ctx *ctx, hipk_dtype dt, int64_t m, int nx, const double *alpha_host,
      const void *X, int64_t ldX, void *Y, int64_t ldY, const void *Z, int64_t ldZ, double *out_dev) {
   if (nx <= 0) return 0;
   if (nx > UTIL_MAXCOLS) return -1;
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(4 * nx)));
   ColScal sc;
   for (int c = 0; c < nx; c++) sc.a[c] = alpha_host[c];
   return reduce_pass(ctx, m, nx, out_dev, [&](int gx) -> int {      /* same grid as hipk_pair_dots: same sums */
      DISPATCH_RT(dt, hipLaunchKernelGGL(axpy_dot_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, sc, (const T *)X, ldX, (T *)Y, ldY, (const T *)Z, ldZ, nx, m, ctx->partials));
      return 0;
   });
}

extern "C" int hipk_qmr_update(hipk_ctx *ctx, hipk_dtype dt, int64_t m, int nx, const double *gamma_host,
      const double *eta_host, const void *D, int64_t ldD, void *Delta, int64_t ldDelta, void *Sol,
      int64_t ldSol, double *dotsol_dev) {
   if (nx <= 0) return 0;
   if (nx > UTIL_MAXCOLS) return -1;
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(5 * nx)));
   ColScal g, e;
   for (int c = 0; c < nx; c++) { g.a[c] = gamma_host[c]; e.a[c] = eta_host[c]; }
   return reduce_pass(ctx, m, nx, dotsol_dev, [&](int gx) -> int {
      DISPATCH_RT(dt, hipLaunchKernelGGL(qmr_update_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, g, e, (const T *)D, ldD, (T *)Delta, ldDelta, (T *)Sol, ldSol, nx, m, ctx->partials));
      return 0;
   });
}

extern "C" int hipk_qmr_update_jacobi(hipk_ctx *ctx, hipk_dtype dt, int64_t m, int nx, const double *gamma_host,
      const double *eta_host, const void *D, int64_t ldD, void *Delta, int64_t ldDelta, void *Sol, int64_t ldSol,
      const void *G, int64_t ldG, const void *diag, const double *shift_host, double min_den, void *W, int64_t ldW,
      double *out_dev) {
   if (nx <= 0) return 0;
   if (nx > UTIL_MAXCOLS) return -1;
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(8 * nx + 1)));
   if (!(min_den > 0.0)) min_den = 1e-300;
   ColScal g, e, sh;
   for (int c = 0; c < nx; c++) { g.a[c] = gamma_host[c]; e.a[c] = eta_host[c]; sh.a[c] = shift_host ? shift_host[c] : 0.0; }
   return reduce_pass(ctx, m, 2 * nx, out_dev, [&](int gx) -> int {
      for (int c0 = 0; c0 < nx; c0 += 8) {
         DISPATCH_RT(dt, hipLaunchKernelGGL(qmr_update_jacobi_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, g, e, sh, min_den, (const T *)D, ldD, (T *)Delta, ldDelta, (T *)Sol, ldSol, (const T *)G, ldG, (const T *)diag, (T *)W, ldW, nx, c0, m, ctx->partials));
         HIPK_CHECK(hipGetLastError());
      }
      return 0;
   });
}

extern "C" int hipk_axpy_proj_dot_jacobi(hipk_ctx *ctx, hipk_dtype dt, int64_t m, int nx, const double *alpha_host, const double *xr_host,
      const void *W, int64_t ldW, const void *X, int64_t ldX, void *G, int64_t ldG, const void *diag, const double *shift_host,
      double min_den, double *out_dev) {
   if (nx <= 0) return 0;
   if (nx > UTIL_MAXCOLS) return -1;
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(4 * nx + 1)));
   if (!(min_den > 0.0)) min_den = 1e-300;
   ColScal a, r, sh;
   for (int c = 0; c < nx; c++) { a.a[c] = alpha_host[c]; r.a[c] = xr_host[c]; sh.a[c] = shift_host ? shift_host[c] : 0.0; }
   QmrPrev pv;
   memset(&pv, 0, sizeof(pv));
   return reduce_pass(ctx, m, 2 * nx, out_dev, [&](int gx) -> int {
      for (int c0 = 0; c0 < nx; c0 += 8) {
         DISPATCH_RT(dt, hipLaunchKernelGGL((axpy_proj_dot_jacobi_kernel<T, false>), dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, a, r, sh, min_den, (const T *)W, ldW, (const T *)X, ldX, (T *)G, ldG, (const T *)diag, nx, c0, m, ctx->partials, (const double *)NULL, pv));
         HIPK_CHECK(hipGetLastError());
      }
      return 0;
   });
}
/* the same with alpha_c = rho_prev_c / (v'w - (x'w)(v'x)) and xr_c = x'w taken from tri_dev = [x'w | v'w | v'x] in HBM (the
 * results of hipk_triple_dots, which the host has NOT seen yet); nx <= 8 */
extern "C" int hipk_axpy_proj_dot_jacobi_dev(hipk_ctx *ctx, hipk_dtype dt, int64_t m, int nx, const double *tri_dev, const double *rho_prev_host,
      double mach_eps, const void *W, int64_t ldW, const void *X, int64_t ldX, void *G, int64_t ldG, const void *diag, const double *shift_host,
      double min_den, double *out_dev) {
   if (nx <= 0) return 0;
   if (nx > 8 || !tri_dev) return -1;
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(4 * nx + 1)));
   if (!(min_den > 0.0)) min_den = 1e-300;
   ColScal z, sh;
   QmrPrev pv;
   memset(&pv, 0, sizeof(pv)); memset(&z, 0, sizeof(z));
   pv.eps = mach_eps;
   for (int c = 0; c < nx; c++) { pv.rho_prev[c] = rho_prev_host[c]; sh.a[c] = shift_host ? shift_host[c] : 0.0; }
   return reduce_pass(ctx, m, 2 * nx, out_dev, [&](int gx) -> int {
      DISPATCH_RT(dt, hipLaunchKernelGGL((axpy_proj_dot_jacobi_kernel<T, true>), dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, z, z, sh, min_den, (const T *)W, ldW, (const T *)X, ldX, (T *)G, ldG, (const T *)diag, nx, 0, m, ctx->partials, tri_dev, pv));
      return 0;
   });
}

extern "C" int hipk_qmr_update_dir(hipk_ctx *ctx, hipk_dtype dt, int64_t m, int nx, const double *gamma_host, const double *eta_host,
      const double *beta_host, void *D, int64_t ldD, void *Delta, int64_t ldDelta, void *Sol, int64_t ldSol, const void *G, int64_t ldG,
      const void *diag, const double *shift_host, double min_den, double *dotsol_dev) {
   if (nx <= 0) return 0;
   if (nx > UTIL_MAXCOLS) return -1;
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(7 * nx + 1)));
   if (!(min_den > 0.0)) min_den = 1e-300;
   ColScal g, e, b, sh;
   for (int c = 0; c < nx; c++) { g.a[c] = gamma_host[c]; e.a[c] = eta_host[c]; b.a[c] = beta_host[c]; sh.a[c] = shift_host ? shift_host[c] : 0.0; }
   QmrPrev pv;
   memset(&pv, 0, sizeof(pv));
   return reduce_pass(ctx, m, nx, dotsol_dev, [&](int gx) -> int {
      for (int c0 = 0; c0 < nx; c0 += 8) {
         DISPATCH_RT(dt, hipLaunchKernelGGL((qmr_update_dir_kernel<T, false>), dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, g, e, b, sh, min_den, (T *)D, ldD, (T *)Delta, ldDelta, (T *)Sol, ldSol, (const T *)G, ldG, (const T *)diag, nx, c0, m, ctx->partials, (const double *)NULL, (const double *)NULL, pv));
         HIPK_CHECK(hipGetLastError());
      }
      return 0;
   });
}
/* the same with gamma, eta, beta of the step formed in the launch from tri_dev (as above), ggr_dev = [g'g | g'K^-1 g] (the results of
 * hipk_axpy_proj_dot_jacobi_dev) and the previous step's rho, tau, Theta; a column whose alpha was unusable is left alone; nx <= 8.
 * dotsol_dev[c] = |sol(:,c)|^2 of the columns that were updated (0 for the others) */
extern "C" int hipk_qmr_update_dir_dev(hipk_ctx *ctx, hipk_dtype dt, int64_t m, int nx, const double *tri_dev, const double *ggr_dev,
      const double *rho_prev_host, const double *tau_prev_host, const double *theta_prev_host, double mach_eps, void *D, int64_t ldD,
      void *Delta, int64_t ldDelta, void *Sol, int64_t ldSol, const void *G, int64_t ldG, const void *diag, const double *shift_host,
      double min_den, double *dotsol_dev) {
   if (nx <= 0) return 0;
   if (nx > 8 || !tri_dev || !ggr_dev) return -1;
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(7 * nx + 1)));
   if (!(min_den > 0.0)) min_den = 1e-300;
   ColScal z, sh;
   QmrPrev pv;
   memset(&pv, 0, sizeof(pv)); memset(&z, 0, sizeof(z));
   pv.eps = mach_eps;
   for (int c = 0; c < nx; c++) {
      pv.rho_prev[c] = rho_prev_host[c]; pv.tau_prev[c] = tau_prev_host[c]; pv.theta_prev[c] = theta_prev_host[c];
      sh.a[c] = shift_host ? shift_host[c] : 0.0;
   }
   return reduce_pass(ctx, m, nx, dotsol_dev, [&](int gx) -> int {
      DISPATCH_RT(dt, hipLaunchKernelGGL((qmr_update_dir_kernel<T, true>), dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, z, z, z, sh, min_den, (T *)D, ldD, (T *)Delta, ldDelta, (T *)Sol, ldSol, (const T *)G, ldG, (const T *)diag, nx, 0, m, ctx->partials, tri_dev, ggr_dev, pv));
      return 0;
   });
}

extern "C" int hipk_triple_dots(hipk_ctx *ctx, hipk_dtype dt, int64_t m, const void *X, int64_t ldX, const void *V, int64_t ldV,
      const void *W, int64_t ldW, int nx, double *out_dev) {
   if (nx <= 0) return 0;
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(3 * nx)));
   return reduce_pass(ctx, m, 3 * nx, out_dev, [&](int gx) -> int {
      DISPATCH_RT(dt, hipLaunchKernelGGL(triple_dots_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, (const T *)X, ldX, (const T *)V, ldV, (const T *)W, ldW, nx, m, ctx->partials));
      return 0;
   });
}

extern "C" int hipk_axpy_proj_dot(hipk_ctx *ctx, hipk_dtype dt, int64_t m, int nx, const double *alpha_host, const double *xr_host,
      const void *W, int64_t ldW, const void *X, int64_t ldX, void *G, int64_t ldG, double *out_dev) {
   if (nx <= 0) return 0;
   if (nx > UTIL_MAXCOLS) return -1;
   hipk_prof_scope ps_(HIPK_PROF_VEC, ctx->stream, hipk_stream_bytes(dt, m, (double)(4 * nx)));
   ColScal a, r;
   for (int c = 0; c < nx; c++) { a.a[c] = alpha_host[c]; r.a[c] = xr_host[c]; }
   return reduce_pass(ctx, m, nx, out_dev, [&](int gx) -> int {
      DISPATCH_RT(dt, hipLaunchKernelGGL(axpy_proj_dot_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, a, r, (const T *)W, ldW, (const T *)X, ldX, (T *)G, ldG, nx, m, ctx->partials));
      return 0;
   });
}

/* ============================ fill, Jacobi preconditioner ================================ */
template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
fill_kernel(T *__restrict__ d, int64_t n, double v) {
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < n; i += stride) d[i] = (T)v;
}

/* d[0..n) = v on the context's stream (library-internal, hipk_internal.h: the diagonal of the stencil operator) */
int hipk_fill(hipk_ctx *ctx, hipk_dtype dt, void *d, int64_t n, double v) {
   const int gx = hipk_grid_for_rows(ctx, n, HIPK_BLOCK * 4, 8);
   DISPATCH_RT(dt, hipLaunchKernelGGL(fill_kernel<T>, dim3(gx), dim3(HIPK_BLOCK), 0, ctx->stream, (T *)d, n, v));
   HIPK_CHECK(hipGetLastError());
   return 0;
}

struct JacShift { double s[64]; };
template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
jacobi_kernel(const T *__restrict__ diag, JacShift sh, double min_den, const T *__restrict__ x, int64_t ldx,
      T *__restrict__ y, int64_t ldy, int ncols, int64_t m) {
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int c = 0; c < ncols; c++) {
      const double shift = sh.s[c];
      for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < m; i += stride) {
         double d = (double)diag[i] - shift;
         /* same guard as the reference's test preconditioner: avoid dividing by ~0 */
         if (fabs(d) <= min_den) d = copysign(min_den, d);           /* a NaN stays a NaN */
         y[i + (size_t)c * ldy] = (T)((double)x[i + (size_t)c * ldx] / d);
      }
   }
}

extern "C" int hipk_jacobi_apply(void *hip_stream, hipk_dtype dt, int64_t m, const void *diag,
      const double *shift_host, double min_den, const void *x, int64_t ldx, void *y, int64_t ldy, int ncols) {
   if (ncols <= 0) return 0;
   if (!(min_den > 0.0)) min_den = 1e-300;
   if (ncols > 64) return -1;
   hipStream_t st = (hipStream_t)hip_stream;
   hipk_prof_scope ps_(HIPK_PROF_VEC, st, (double)m * (double)hipk_elem_size(dt) * (2.0 * ncols) + (double)m * (double)hipk_elem_size(hipk_real_of(dt)));
   static int num_cu = 0;                      /* launch geometry only: read the device once */
   if (num_cu == 0) {
      int dev = 0, n = 0;
      if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) num_cu = n;
      else num_cu = 256;
   }
   if (HIPK_IS_Z(dt)) return hipk_z_jacobi(st, num_cu, dt, m, diag, shift_host, min_den, x, ldx, y, ldy, ncols);
   if (dt != HIPK_F64 && dt != HIPK_F32) return -44;
   JacShift sh;
   for (int c = 0; c < ncols; c++) sh.s[c] = shift_host ? shift_host[c] : 0.0;
   const int64_t need = (m + HIPK_BLOCK * 4 - 1) / (HIPK_BLOCK * 4);
   const int gx = (int)(need < 1 ? 1 : (need < (int64_t)num_cu * 8 ? need : (int64_t)num_cu * 8));
   if (dt == HIPK_F64)
      hipLaunchKernelGGL(jacobi_kernel<double>, dim3(gx), dim3(HIPK_BLOCK), 0, st, (const double *)diag, sh, min_den, (const double *)x, ldx, (double *)y, ldy, ncols, m);
   else
      hipLaunchKernelGGL(jacobi_kernel<float>, dim3(gx), dim3(HIPK_BLOCK), 0, st, (const float *)diag, sh, min_den, (const float *)x, ldx, (float *)y, ldy, ncols, m);
   const hipError_t e = hipGetLastError();
   if (e != hipSuccess) { fprintf(stderr, "primme_amd: jacobi_kernel launch failed: %s\n", hipGetErrorString(e)); return -1; }
   return 0;
}
