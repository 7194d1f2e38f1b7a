/* members.h — the table-driven member interface shared by eigs_members.c (primme_params) and svds_members.c
 * (primme_svds_params): one row per label says where the member lies and how it travels through `value`; the same rows serve
 * get, set, member_info, enum_member_info and the display routines.  The engine is in eigs_members.c. */
#ifndef PA_MEMBERS_H
#define PA_MEMBERS_H

#include <stddef.h>
#include <stdio.h>
#include "primme_amd_svds.h"

/* how a member is stored and what `value` is in get / set */
typedef enum {
   PA_MK_INT,      /* int member; value: PRIMME_INT*, set refuses values above INT_MAX            -> primme_int     */
   PA_MK_ENUM,     /* enum member (an int wide); value: PRIMME_INT*, set truncates like a C cast  -> primme_int     */
   PA_MK_LONG,     /* PRIMME_INT member; value: PRIMME_INT*                                       -> primme_int     */
   PA_MK_LONG4,    /* PRIMME_INT[4] (iseed); value: PRIMME_INT[4]                                 -> primme_int     */
   PA_MK_DOUBLE,   /* double member; value: double*                                               -> primme_double  */
   PA_MK_DARRAY,   /* double* member; set: value IS the pointer, get: stored through (void **)    -> primme_double  */
   PA_MK_POINTER,  /* data or function pointer; as PA_MK_DARRAY                                   -> primme_pointer */
   PA_MK_STRING,   /* const char*; as PA_MK_DARRAY                                                -> primme_string  */
   PA_MK_NESTED    /* a nested structure: get gives its address, set refuses                      -> primme_pointer */
} pa_member_kind;

/* what the reference does not serve for a member (restated, not repaired) */
enum { PA_MF_NO_GET = 1, PA_MF_NO_SET = 2 };

/* enumerations; a member's `enumeration` is what ?_enum_member_info answers for it (0: none) */
enum {
   PA_EN_NONE = 0, PA_EN_METHOD, PA_EN_TARGET, PA_EN_PROJECTION, PA_EN_INIT, PA_EN_CONVTEST, PA_EN_EVENT, PA_EN_ORTH, PA_EN_OP,
   PA_EN_SVDS_METHOD, PA_EN_SVDS_TARGET, PA_EN_SVDS_OPERATOR
};

typedef struct {
   int label;           /* primme_params_label / primme_svds_params_label */
   const char *name;    /* the reference's name of the label; NULL: member_info does not know the label */
   const char *path;    /* the member as C writes it, nested structures joined with '.' */
   size_t offset;
   unsigned char kind, arity, flags, enumeration;
} pa_member;

typedef struct {
   const char *name;
   int value;
   unsigned char enumeration;
   unsigned char silent;   /* the display routines print nothing for this value */
} pa_constant;

/* one line of a configuration listing */
typedef enum {
   PA_DS_TEXT,     /* `text` as it is */
   PA_DS_INT,      /* prefix.member = %d (or PRIMME_INT_P: the same digits) */
   PA_DS_E,        /* prefix.member = %e */
   PA_DS_G,        /* prefix.member = %g */
   PA_DS_ENUM,     /* prefix.member = enumerator name; `enumeration` says which */
   PA_DS_SHIFTS,   /* prefix.member = the `count` doubles behind the pointer, when count > 0 */
   PA_DS_SEED      /* prefix.member = the four integers */
} pa_display_style;
typedef struct { unsigned char style; int label; int aux; const char *text; } pa_display_line;   /* aux: enumeration / label of the count */

const pa_member *pa_member_find(const pa_member *table, int rows, int label);
int pa_member_get(const pa_member *table, int rows, void *base, int label, void *value);
int pa_member_set(const pa_member *table, int rows, void *base, int label, void *value);
int pa_member_info(const pa_member *table, int rows, int *label, const char **label_name, primme_type *type, int *arity);
int pa_constant_info(const pa_constant *constants, int count, const char *name, int *value);
int pa_enum_member_info(const pa_member *table, int rows, const pa_constant *constants, int count, int label, int *value,
      const char **value_name);
void pa_display(FILE *out, const char *prefix, const pa_member *table, int rows, void *base, const pa_display_line *lines,
      int nlines, const pa_constant *constants, int count);

/* primme_params under another prefix: primme_svds_display_params lists its two stages with it */
void pa_display_eigs(FILE *out, const char *prefix, primme_params *primme);

#endif
