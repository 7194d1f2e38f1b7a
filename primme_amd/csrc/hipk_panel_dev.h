/* hipk_panel_dev.h — what the panel kernel families (hipk_panels.hip, hipk_ritz.hip, hipk_vec.hip) share: the
 * column-segment argument record, 16-byte lane vectors, the streamed (non-temporal) loads and stores, the alignment
 * tests of their launchers and the limits of the by-value kernel arguments.  Included by .hip files only. */
#ifndef HIPK_PANEL_DEV_H
#define HIPK_PANEL_DEV_H

#include "hipk_internal.h"
#include <cstddef>

struct SegArgs {
   const void *base[HIPK_MAX_SEGS];
   int64_t ld[HIPK_MAX_SEGS];
   int n[HIPK_MAX_SEGS];
   int total;
};

static inline int pack_segs(const hipk_seg *segs, int nseg, SegArgs *a) {
   if (nseg < 0 || nseg > HIPK_MAX_SEGS) return -1;
   a->total = 0;
   for (int s = 0; s < HIPK_MAX_SEGS; s++) {
      if (s < nseg && segs[s].ncols > 0) {
         a->base[s] = segs[s].base; a->ld[s] = segs[s].ld; a->n[s] = segs[s].ncols;
      } else {
         a->base[s] = NULL; a->ld[s] = 0; a->n[s] = 0;
      }
      a->total += a->n[s];
   }
   return 0;
}

/* 16-byte lane accesses: VW consecutive rows per lane (2 doubles / 4 floats) when every
 * column involved is 16-byte aligned, VW = 1 otherwise */
template <typename T, int VW> struct lanevec { T e[VW]; };
template <> struct __attribute__((aligned(16))) lanevec<double, 2> { double e[2]; };
template <> struct __attribute__((aligned(16))) lanevec<float, 4> { float e[4]; };
template <> struct __attribute__((aligned(8))) lanevec<float, 2> { float e[2]; };
template <typename T> struct vecwidth { enum { value = 16 / sizeof(T) }; };
/* Streamed panels are loaded (and the restart pass' outputs stored) with the NON-TEMPORAL hint: V and W are read once per
 * kernel and are far larger than the 256 MiB Infinity Cache, so letting them allocate there only evicts what does get
 * re-read every iteration — the CSR matrix and the vectors of the SpMV (215 MB at n = 2 M).  Measured on one box, back to
 * back (profiles/r03_nontemporal_ab.log): configs[1] 13.72 -> 14.82 eigenpairs/s (SpMV 146 -> 124 ms per solve: it now
 * hits the cache; fused residual / restart class 4.96 -> 5.44 TB/s), north-star workload 2.466 -> 2.321 s per 3000
 * iterations.  HIPK_NT_LOADS is a build-time mask for A/B builds (scripts/build_variant.sh): 1 = W in the fused
 * residual kernel, 2 = V, Q there and the panels of the Gram-Schmidt update, 4 = loads of the restart kernels,
 * 8 = stores of the restart pass, 16 = panels of the TN kernel (no gain: left off).  Default 15. */
#ifndef HIPK_NT_LOADS
#define HIPK_NT_LOADS 15
#endif
template <typename T, int NTBIT>
__device__ __forceinline__ T ldstream1(const T *p) {
   if ((HIPK_NT_LOADS & NTBIT) != 0) return __builtin_nontemporal_load(p);
   return *p;
}
template <typename T, int NTBIT>
__device__ __forceinline__ void ststream1(T *p, T v) {
   if ((HIPK_NT_LOADS & NTBIT) != 0) __builtin_nontemporal_store(v, p);
   else *p = v;
}
template <typename T, int VW, int NTBIT>
__device__ __forceinline__ lanevec<T, VW> ldstream(const T *col, int64_t idx) {
   if ((HIPK_NT_LOADS & NTBIT) != 0) {
      typedef T nvec __attribute__((ext_vector_type(VW)));
      const nvec t = __builtin_nontemporal_load((const nvec *)col + idx);
      lanevec<T, VW> r;
#pragma unroll
      for (int i = 0; i < VW; i++) r.e[i] = t[i];
      return r;
   }
   return ((const lanevec<T, VW> *)col)[idx];
}

static inline bool aligned16(const void *p, int64_t ld, size_t es) {
   return (((uintptr_t)p) & 15) == 0 && ((ld * (int64_t)es) & 15) == 0;
}
static inline bool segs_aligned16(const SegArgs &a, size_t es) {
   for (int s = 0; s < HIPK_MAX_SEGS; s++)
      if (a.n[s] > 0 && !aligned16(a.base[s], a.ld[s], es)) return false;
   return true;
}

template <typename T>
__device__ __forceinline__ const T *seg_col(const SegArgs &s, int j) {
   int q = 0;
   if (j >= s.n[0]) { j -= s.n[0]; q = 1; if (j >= s.n[1]) { j -= s.n[1]; q = 2; } }
   return (const T *)s.base[q] + (size_t)j * (size_t)s.ld[q];
}

/* basis columns one launch of the Gram-Schmidt kernels stages in LDS; widest workgroup of a finishing launch */
#define PROJ_MAXCOLS 192
#define FIN_TAIL_MAXBLOCK 1024

/* per-column host scalars / a column permutation travel in the kernel arguments, UTIL_MAXCOLS columns per launch */
#define UTIL_MAXCOLS 64
struct ColScal { double a[UTIL_MAXCOLS]; };
struct ColPerm { int p[UTIL_MAXCOLS]; };

#endif
