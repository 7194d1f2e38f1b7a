/* hipk_cheb.hip — device pieces of the Chebyshev polynomial preconditioner K^-1 = p(A) (gfx950).
 *
 * p(A) x is the d-th iterate of Chebyshev iteration for (A - sigma I) y = x started from y = 0, with [lo, hi] the part of
 * the spectrum to damp ("Chebyshev polynomial preconditioner"; the callback and the host recurrence of the
 * coefficients are in amd_operator.hip).  Every step is one linear combination per row,
 *      y_{k+1}(i) = cy y_k(i) + cp y_{k-1}(i) + cx x(i) + cw (A y_k)(i),
 * with four REAL coefficients per column (hipk_cheb_coef; the shift sigma is folded into cy).  Two ways to run it:
 *   generic   the operator product into a scratch panel (primme_amd_operator_apply: every operator form, halo exchange
 *             included), then cheb_update_kernel below: one pass, 16-byte accesses, 5 vector streams per row and column;
 *   fused     the product and the combination in one pass — an epilogue of the row-pattern kernel (hipk_sparse_pat.hip)
 *             and of the windowed CSR tile kernel (hipk_sparse.hip), entry point hipk_csr_cheb_step there.
 * Also here: the Gershgorin bounds of a CSR slab (one pass over the matrix), which give the upper end of the interval.
 * No reference counterpart: the reference ships no preconditioner, its test driver has diagonal and ILUT ones on the host
 * (tests/COMMON/mat.c). */
#include "hipk_internal.h"

/* VW consecutive elements moved as one access (16 bytes when the panels allow it) */
template <typename T, int VW> struct alignas(sizeof(T) * VW) cheb_pack { T v[VW]; };

/* Out(:,c) = cy[c] Yk(:,c) + cp[c] Yp(:,c) + cx[c] X(:,c) + cw[c] W(:,c); a NULL panel is left out.  Row-local: Out may be
 * any of the inputs.  blockIdx.y = column.  Arithmetic in double whatever T is (the coefficients are doubles). */
template <typename T, int VW>
__global__ void __launch_bounds__(HIPK_BLOCK)
cheb_update_kernel(int64_t m, hipk_cheb_coef cf, const T *X, int64_t ldx, const T *W, int64_t ldw, const T *Yk, int64_t ldk,
      const T *Yp, int64_t ldp, T *Out, int64_t ldo) {
   typedef cheb_pack<T, VW> P;
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
      if (w) pw = ((const P *)w)[i];
      if (yk) pk = ((const P *)yk)[i];
      if (yp) pp = ((const P *)yp)[i];
#pragma unroll
      for (int e = 0; e < VW; e++) {
         double s = cx * (double)px.v[e];
         if (yk) s = fma(cy, (double)pk.v[e], s);
         if (yp) s = fma(cp, (double)pp.v[e], s);
         if (w) s = fma(cw, (double)pw.v[e], s);
         po.v[e] = (T)s;
      }
      ((P *)out)[i] = po;
   }
   /* the rows past the last full access */
   for (int64_t i = nv * VW + gid; i < m; i += stride) {
      double s = cx * (double)x[i];
      if (yk) s = fma(cy, (double)yk[i], s);
      if (yp) s = fma(cp, (double)yp[i], s);
      if (w) s = fma(cw, (double)w[i], s);
      out[i] = (T)s;
   }
}

static int cheb_num_cu(void) {
   static int num_cu = 0;                      /* launch geometry only: read the device once */
   if (num_cu == 0) {
      int dev = 0, n = 0;
      if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) num_cu = n;
      else num_cu = 256;
   }
   return num_cu;
}

static bool cheb_al16(const void *p, int64_t ld, size_t es) { return !p || (((uintptr_t)p & 15) == 0 && ((size_t)ld * es) % 16 == 0); }

template <typename T>
static int cheb_update_t(hipStream_t st, int64_t m, int nx, const hipk_cheb_coef &cf, const T *X, int64_t ldx, const T *W, int64_t ldw,
      const T *Yk, int64_t ldk, const T *Yp, int64_t ldp, T *Out, int64_t ldo) {
   constexpr int VW = 16 / sizeof(T);
   const bool vec = cheb_al16(X, ldx, sizeof(T)) && cheb_al16(W, ldw, sizeof(T)) && cheb_al16(Yk, ldk, sizeof(T)) &&
                    cheb_al16(Yp, ldp, sizeof(T)) && cheb_al16(Out, ldo, sizeof(T));
   const int64_t per = (int64_t)HIPK_BLOCK * (vec ? VW : 1) * 2;                 /* two trips per lane */
   int64_t gx = (m + per - 1) / per;
   const int64_t cap = (int64_t)cheb_num_cu() * 8;
   if (gx > cap) gx = cap;
   if (gx < 1) gx = 1;
   if (vec) hipLaunchKernelGGL((cheb_update_kernel<T, VW>), dim3((unsigned)gx, nx), dim3(HIPK_BLOCK), 0, st, m, cf, X, ldx, W, ldw, Yk, ldk, Yp, ldp, Out, ldo);
   else hipLaunchKernelGGL((cheb_update_kernel<T, 1>), dim3((unsigned)gx, nx), dim3(HIPK_BLOCK), 0, st, m, cf, X, ldx, W, ldw, Yk, ldk, Yp, ldp, Out, ldo);
   HIPK_CHECK(hipGetLastError());
   return 0;
}

extern "C" int hipk_cheb_update(void *hip_stream, hipk_dtype dt, int64_t m, int nx, const hipk_cheb_coef *coef, const void *X, int64_t ldx,
      const void *W, int64_t ldw, const void *Yk, int64_t ldk, const void *Yprev, int64_t ldp, void *Out, int64_t ldo) {
   if (nx <= 0 || m <= 0) return 0;
   if (nx > HIPK_CHEB_MAXCOLS || !coef || !X || !Out) return -1;
   hipStream_t st = (hipStream_t)hip_stream;
   /* the coefficients are real: a complex panel is updated as the 2m reals it is made of */
   const int f = HIPK_IS_Z(dt) ? 2 : 1;
   const hipk_dtype rt = hipk_real_of(dt);
   int nin = 1 + (W != NULL) + (Yk != NULL) + (Yprev != NULL);
   hipk_prof_scope ps_(HIPK_PROF_VEC, st, hipk_stream_bytes(dt, m, (double)nx * (nin + 1)));
   if (rt == HIPK_F64)
      return cheb_update_t<double>(st, m * f, nx, *coef, (const double *)X, ldx * f, (const double *)W, ldw * f, (const double *)Yk, ldk * f,
            (const double *)Yprev, ldp * f, (double *)Out, ldo * f);
   return cheb_update_t<float>(st, m * f, nx, *coef, (const float *)X, ldx * f, (const float *)W, ldw * f, (const float *)Yk, ldk * f,
         (const float *)Yprev, ldp * f, (float *)Out, ldo * f);
}

/* ---- Gershgorin bounds of a CSR slab --------------------------------------------------------------------------
 * part[2 b] = min over the rows of workgroup b of (a_ii - sum_{j != i} |a_ij|), part[2 b + 1] = max of (a_ii + sum ...);
 * one lane per row (the diagonal of a Hermitian matrix is real: its real part is taken), CPLX: values are (re, im) pairs */
template <typename T, bool CPLX>
__global__ void __launch_bounds__(HIPK_BLOCK)
cheb_gershgorin_kernel(int64_t nrows, int64_t row0, const int32_t *__restrict__ rowptr, const int32_t *__restrict__ colind,
      const T *__restrict__ val, double *__restrict__ part) {
   __shared__ double smin[HIPK_BLOCK / HIPK_WAVE], smax[HIPK_BLOCK / HIPK_WAVE];
   double lo = INFINITY, hi = -INFINITY;
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < nrows; i += stride) {
      double d = 0.0, s = 0.0;
      for (int32_t q = rowptr[i]; q < rowptr[i + 1]; q++) {
         const double re = CPLX ? (double)val[2 * (size_t)q] : (double)val[q];
         if ((int64_t)colind[q] == row0 + i) d += re;
         else s += CPLX ? hypot(re, (double)val[2 * (size_t)q + 1]) : fabs(re);
      }
      lo = fmin(lo, d - s);
      hi = fmax(hi, d + s);
   }
   for (int o = 32; o > 0; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o)); hi = fmax(hi, __shfl_xor(hi, o)); }
   if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
   __syncthreads();
   if (threadIdx.x == 0) {
      part[2 * blockIdx.x] = fmin(fmin(smin[0], smin[1]), fmin(smin[2], smin[3]));
      part[2 * blockIdx.x + 1] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
   }
}
/* second stage: one workgroup folds the nb pairs into out[0], out[1] */
__global__ void __launch_bounds__(HIPK_BLOCK)
cheb_minmax_kernel(const double *__restrict__ part, int nb, double *__restrict__ out) {
   __shared__ double smin[HIPK_BLOCK / HIPK_WAVE], smax[HIPK_BLOCK / HIPK_WAVE];
   double lo = INFINITY, hi = -INFINITY;
   for (int b = threadIdx.x; b < nb; b += HIPK_BLOCK) { lo = fmin(lo, part[2 * b]); hi = fmax(hi, part[2 * b + 1]); }
   for (int o = 32; o > 0; o >>= 1) { lo = fmin(lo, __shfl_xor(lo, o)); hi = fmax(hi, __shfl_xor(hi, o)); }
   if ((threadIdx.x & 63) == 0) { smin[threadIdx.x >> 6] = lo; smax[threadIdx.x >> 6] = hi; }
   __syncthreads();
   if (threadIdx.x == 0) {
      out[0] = fmin(fmin(smin[0], smin[1]), fmin(smin[2], smin[3]));
      out[1] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
   }
}

/* library-internal (hipk_csr_gershgorin in hipk_sparse.hip owns the matrix): bounds of the rows of one slab, complete on
 * return; an empty slab gives [+inf, -inf], the neutral element of the reduction across ranks */
int hipk_cheb_gershgorin_rows(hipk_ctx *ctx, hipStream_t st, hipk_dtype dt, int64_t nrows, int64_t row0, const int32_t *rowptr,
      const int32_t *colind, const void *val, double out[2]) {
   out[0] = INFINITY; out[1] = -INFINITY;
   if (nrows <= 0) return 0;
   const int gx = hipk_grid_for_rows(ctx, nrows, HIPK_BLOCK, 8);
   double *part = NULL;
   HIPK_CHECK(hipMalloc((void **)&part, sizeof(double) * (2 * (size_t)gx + 2)));
   switch (dt) {
   case HIPK_F64: hipLaunchKernelGGL((cheb_gershgorin_kernel<double, false>), dim3(gx), dim3(HIPK_BLOCK), 0, st, nrows, row0, rowptr, colind, (const double *)val, part); break;
   case HIPK_F32: hipLaunchKernelGGL((cheb_gershgorin_kernel<float, false>), dim3(gx), dim3(HIPK_BLOCK), 0, st, nrows, row0, rowptr, colind, (const float *)val, part); break;
   case HIPK_C64: hipLaunchKernelGGL((cheb_gershgorin_kernel<double, true>), dim3(gx), dim3(HIPK_BLOCK), 0, st, nrows, row0, rowptr, colind, (const double *)val, part); break;
   default: hipLaunchKernelGGL((cheb_gershgorin_kernel<float, true>), dim3(gx), dim3(HIPK_BLOCK), 0, st, nrows, row0, rowptr, colind, (const float *)val, part); break;
   }
   hipLaunchKernelGGL(cheb_minmax_kernel, dim3(1), dim3(HIPK_BLOCK), 0, st, part, gx, part + 2 * (size_t)gx);
   /* `out` is the caller's memory (a stack variable, a ctypes buffer): the result comes back through the context's pinned
    * staging buffer like every other read-back (hipk_download), never by an asynchronous copy into pageable pages */
   hipError_t e = hipGetLastError();
   if (e == hipSuccess) e = hipStreamSynchronize(st);
   double res[2] = {INFINITY, -INFINITY};
   const int rc = e == hipSuccess ? hipk_download(ctx, res, part + 2 * (size_t)gx, sizeof(res)) : -1;
   (void)hipFree(part);
   if (e != hipSuccess || rc) { fprintf(stderr, "primme_amd: Gershgorin reduction failed: %s\n", e != hipSuccess ? hipGetErrorString(e) : "read-back"); return -1; }
   out[0] = res[0]; out[1] = res[1];
   return 0;
}

/* ---- largest absolute row sum of a CSR slab ---------------------------------------------------------------------
 * part[b] = max over the rows of workgroup b of sum_j |a_ij| (one lane per row, the entries added in row order in double);
 * the second stage folds the partial maxima in a fixed order.  A maximum does not depend on the order anyway: the result is
 * the same on every grid. */
template <typename T>
__global__ void __launch_bounds__(HIPK_BLOCK)
cheb_abs_rowsum_kernel(int64_t nrows, const int32_t *__restrict__ rowptr, const T *__restrict__ val, double *__restrict__ part) {
   __shared__ double smax[HIPK_BLOCK / HIPK_WAVE];
   double hi = 0.0;
   const int64_t stride = (int64_t)gridDim.x * HIPK_BLOCK;
   for (int64_t i = (int64_t)blockIdx.x * HIPK_BLOCK + threadIdx.x; i < nrows; i += stride) {
      double s = 0.0;
      for (int32_t q = rowptr[i]; q < rowptr[i + 1]; q++) s += fabs((double)val[q]);
      hi = fmax(hi, s);
   }
   for (int o = 32; o > 0; o >>= 1) hi = fmax(hi, __shfl_xor(hi, o));
   if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = hi;
   __syncthreads();
   if (threadIdx.x == 0) part[blockIdx.x] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
}
__global__ void __launch_bounds__(HIPK_BLOCK)
cheb_max_kernel(const double *__restrict__ part, int nb, double *__restrict__ out) {
   __shared__ double smax[HIPK_BLOCK / HIPK_WAVE];
   double hi = 0.0;
   for (int b = threadIdx.x; b < nb; b += HIPK_BLOCK) hi = fmax(hi, part[b]);
   for (int o = 32; o > 0; o >>= 1) hi = fmax(hi, __shfl_xor(hi, o));
   if ((threadIdx.x & 63) == 0) smax[threadIdx.x >> 6] = hi;
   __syncthreads();
   if (threadIdx.x == 0) out[0] = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
}

/* library-internal (hipk_csr_abs_rowsum_max in hipk_sparse.hip owns the matrix); complete on return, 0 for an empty slab */
int hipk_cheb_abs_rowsum_rows(hipk_ctx *ctx, hipStream_t st, hipk_dtype dt, int64_t nrows, const int32_t *rowptr, const void *val, double *out) {
   *out = 0.0;
   if (nrows <= 0) return 0;
   const int gx = hipk_grid_for_rows(ctx, nrows, HIPK_BLOCK, 8);
   double *part = NULL;
   HIPK_CHECK(hipMalloc((void **)&part, sizeof(double) * ((size_t)gx + 1)));
   if (dt == HIPK_F64) hipLaunchKernelGGL(cheb_abs_rowsum_kernel<double>, dim3(gx), dim3(HIPK_BLOCK), 0, st, nrows, rowptr, (const double *)val, part);
   else hipLaunchKernelGGL(cheb_abs_rowsum_kernel<float>, dim3(gx), dim3(HIPK_BLOCK), 0, st, nrows, rowptr, (const float *)val, part);
   hipLaunchKernelGGL(cheb_max_kernel, dim3(1), dim3(HIPK_BLOCK), 0, st, part, gx, part + gx);
   hipError_t e = hipGetLastError();
   if (e == hipSuccess) e = hipStreamSynchronize(st);
   double res = 0.0;
   const int rc = e == hipSuccess ? hipk_download(ctx, &res, part + gx, sizeof(res)) : -1;
   (void)hipFree(part);
   if (e != hipSuccess || rc) { fprintf(stderr, "primme_amd: row-sum reduction failed: %s\n", e != hipSuccess ? hipGetErrorString(e) : "read-back"); return -1; }
   *out = res;
   return 0;
}
