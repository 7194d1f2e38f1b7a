/* primme.h — the header name the reference's applications include.
 *
 * Umbrella over primme_amd.h (eigenvalue problems) and primme_amd_svds.h (singular value problems) that adds what those
 * programs expect from the reference's include/primme.h: the integer type with its printf conversion and maximum, the complex
 * types, the version numbers and the failure codes.  A program written against the reference's CPU library compiles with
 * -I include and links with -lprimme_amd as it is.
 *
 * PRIMME_INT_SIZE = 64 (default), 32 or 0 (plain int) selects PRIMME_INT as in the reference.  The library itself is built
 * with the 64-bit default; the other widths change the structure layout and are only for code that is compiled against the
 * headers without calling the library.  primme_amd.h may be included before this header; PRIMME_INT is then already int64_t.
 */
#ifndef PRIMME_H
#define PRIMME_H

#define PRIMME_VERSION_MAJOR 3
#define PRIMME_VERSION_MINOR 2

#ifdef __cplusplus
#  include <complex>
#  define PRIMME_COMPLEX_FLOAT std::complex<float>
#  define PRIMME_COMPLEX_DOUBLE std::complex<double>
#else
#  include <complex.h>
#  define PRIMME_COMPLEX_FLOAT float complex
#  define PRIMME_COMPLEX_DOUBLE double complex
#endif

#if defined(__cplusplus) && !defined(__STDC_FORMAT_MACROS)
#  define __STDC_FORMAT_MACROS /* C++ compilers before C++11 hide PRId64 without it */
#endif
#include <inttypes.h>
#include <limits.h>
#include <stdint.h>

#if defined(PRIMME_AMD_H) || !defined(PRIMME_INT_SIZE) || PRIMME_INT_SIZE == 64
#  ifndef PRIMME_INT
#    define PRIMME_INT int64_t
#  endif
#  define PRIMME_INT_P PRId64
#  define PRIMME_INT_MAX INT64_MAX
#elif PRIMME_INT_SIZE == 32
#  define PRIMME_INT int32_t
#  define PRIMME_INT_P PRId32
#  define PRIMME_INT_MAX INT32_MAX
#elif PRIMME_INT_SIZE == 0
#  define PRIMME_INT int
#  define PRIMME_INT_P "d"
#  define PRIMME_INT_MAX INT_MAX
#else
#  error "PRIMME_INT_SIZE must be 64, 32 or 0"
#endif

/* the structures, enums and entry points */
#include "primme_amd.h"
#include "primme_amd_svds.h"

/* the failure codes of the solvers (primme_amd.h has them for the programs that include it alone) */
#ifndef PRIMME_UNEXPECTED_FAILURE
#  define PRIMME_UNEXPECTED_FAILURE   (-1)
#  define PRIMME_MALLOC_FAILURE       (-2)
#  define PRIMME_MAIN_ITER_FAILURE    (-3)
#  define PRIMME_LAPACK_FAILURE       (-40)
#  define PRIMME_USER_FAILURE         (-41)
#  define PRIMME_ORTHO_CONST_FAILURE  (-42)
#  define PRIMME_PARALLEL_FAILURE     (-43)
#  define PRIMME_FUNCTION_UNAVAILABLE (-44)
#endif

#endif /* PRIMME_H */
