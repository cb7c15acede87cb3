/* sparse_rx_fields.h -- field predicates: filter rows built on the device from resident metadata columns.
 *
 * Ninth header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: sparse_rx_filter.h names four uses of a doc filter -- tombstones, a tenant's docs, the result of a metadata predicate,
 * "not the ones already shown".  Three of them have a builder on the device (srx_filter_set_docs, srx_filter_fill,
 * srx_filter_from_terms); the metadata predicate ("published since 2023", "source is wiki or arxiv", "tenant = 17 and not
 * tagged draft", "price below 50") had to be evaluated over the whole corpus on the host, packed and uploaded, per request.
 * This header turns typed columns that stay resident and a small predicate into filter rows.  It is a builder, not a
 * search: the rows go to every filtered search as they are.  The reference's Document carries a metadata dict that nothing
 * reads: nothing here replaces reference code.
 *
 * ---- the contract -----------------------------------------------------------------------------------------------------
 *
 * Columns      n_cols (1 .. 32) descriptors in a HOST array; each names a device array of n_docs values of its type,
 *              naturally aligned (I32 / F32: 4 bytes, I64 / SET64: 8 bytes), and optionally ONE filter row `valid`
 *              (as many words as srx_filter_words gives for n_docs, 16-byte aligned): bit d set = doc d has a value; NULL = every doc has one.
 *              A SET64 value is a set of up to 64 labels, label i = bit i.
 * Clauses      a DEVICE array of n_clauses records of 24 bytes: (col, op, lo, hi).  Clause c HOLDS for doc d iff d has a
 *              value in cols[c.col] and the test passes on that value v:
 *                RANGE      lo <= v <= hi.  I32 and I64 columns: a signed compare of 64-bit integers -- an I32 value is
 *                           widened, the bounds are not narrowed.  F32 columns: lo and hi hold the bits of a float in
 *                           their low 32 bits, and the compares are IEEE (a NaN value passes no range, a NaN bound
 *                           admits nothing, -0 == +0).  lo > hi is a legal clause that no doc passes.
 *                IN         v equals one of values[lo .. lo + hi).  Integer columns compare as int64; F32 columns compare
 *                           the float whose bits are the low 32 of the entry, by IEEE == (NaN equals nothing).  hi == 0
 *                           passes no doc.
 *                MASK_ANY   (v & lo) != 0.         SET64 columns only.
 *                MASK_ALL   (v & lo) == lo.        SET64 columns only (lo == 0 passes every doc that has a value).
 *              RANGE and IN are not for SET64 columns, MASK_* not for the others.
 * Lists        three ragged lists of clause ids per output row, each a device CSR: ptr i32[n_rows + 1] (ptr[0] = 0, ascending)
 *              and clause i32[ptr[n_rows]].  A list is absent for every row when BOTH its pointers are NULL.
 * Row r allows local doc d (0 <= d < n_docs) iff all of
 *                base(r, d)            the base filter's row q_filter[r] allows d (q_filter NULL: row 0; -1: every doc; a NULL
 *                                      base: every doc) -- base->q_filter is read per OUTPUT row, i32[n_rows], as in
 *                                      srx_filter_from_terms;
 *                all[r]                every clause of the list holds;
 *                any[r]                the list is empty, or one of its clauses holds;
 *                none[r]               no clause of the list holds.
 *              A doc without a value therefore fails a clause in `all` and passes it in `none`.  A row with three empty
 *              lists is the base row (or every doc).  The clause table is shared by the rows; duplicate ids are legal; a
 *              clause in both `all` and `none` gives an empty row.
 * Clause ids   -1 is legal in every list and means "a clause no doc satisfies" (the host's spelling of an unknown category),
 *              read like the -1 term id of srx_filter_from_terms: in `all` it makes the row empty, in `any` it contributes
 *              nothing but the list counts as non-empty, in `none` it has no effect.
 * Preconditions, NOT checked on the device: a clause id outside [-1, n_clauses); a col outside [0, n_cols); an op that does
 *              not fit the column's type; an IN range outside `values`; a q_filter value outside [-1, n_filters).  For the
 *              first three the kernel treats the clause as one no doc satisfies: it makes no wild read.
 * Output       every word of every row is written: out_bits u32[n_rows][words], words = srx_filter_words of n_docs -- its
 *              size in bytes is what srx_filter_from_terms_bytes of sparse_rx_terms.h returns for (n_rows, n_docs); bits at or above n_docs
 *              and the padding words are 0 (the row contract of srx_filter_fill).  out_bits must not overlap base->bits or
 *              any `valid` row.
 * The call is asynchronous on `stream`, allocates nothing, needs no workspace and uses no global atomics.  The columns, the
 * validity rows, the clauses, the lists and `values` are only read; they must not be written while a call that uses them is
 * in flight.
 *
 * Refused with SRX_ERR_INVALID before anything touches a device: n_docs outside [1, 2^31 - 2]; n_cols outside [1, 32]; a
 * NULL cols; a column with a NULL data, or data misaligned for its type; an unknown column type; a misaligned (16 bytes)
 * valid; n_clauses < 0, or a NULL clauses with n_clauses > 0; n_rows < 0; one pointer of a ptr / clause pair NULL without
 * the other; a NULL or misaligned (16 bytes) out_bits; a base that srx_search_filtered would refuse (NULL or misaligned
 * bits, n_filters < 1).  n_rows == 0 returns SRX_OK without a launch.
 *
 * Not covered: strings on the device (a category is its code, the dictionary stays with the host), more than 64 labels per
 * set column, prefix or regex tests, updating single values in place, a sharded index (rows are shard-local, as every
 * filter's).
 */
#ifndef SPARSE_RX_FIELDS_H
#define SPARSE_RX_FIELDS_H

#include "sparse_rx_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SRX_FIELD_I32 = 0, SRX_FIELD_I64 = 1, SRX_FIELD_F32 = 2, SRX_FIELD_SET64 = 3 };  /* column types */
enum { SRX_FOP_RANGE = 0, SRX_FOP_IN = 1, SRX_FOP_MASK_ANY = 2, SRX_FOP_MASK_ALL = 3 }; /* clause ops   */

typedef struct srx_field_col { /* HOST struct */
    const void *data;          /* device, [n_docs] of the type, naturally aligned */
    const uint32_t *valid;     /* device, ONE filter row, 16-byte aligned; NULL = every doc has a value */
    int32_t type;
} srx_field_col;

typedef struct srx_field_clause { /* DEVICE array element, 24 bytes */
    int32_t col, op;
    int64_t lo; /* RANGE: inclusive low bound (F32 column: the float's bits in the low 32); MASK_*: the 64-bit mask; IN: first index into values */
    int64_t hi; /* RANGE: inclusive high bound; IN: how many values */
} srx_field_clause;

int srx_filter_from_fields(int32_t device, int64_t n_docs,
                           const srx_field_col *cols, int32_t n_cols,            /* host array, 1 <= n_cols <= 32 */
                           const srx_field_clause *clauses, int32_t n_clauses,   /* device */
                           const int64_t *values,                                /* device, the IN lists; NULL when no clause is IN */
                           int32_t n_rows,
                           const int32_t *all_ptr, const int32_t *all_clause,    /* device CSR of clause ids; both NULL = no such list */
                           const int32_t *any_ptr, const int32_t *any_clause,
                           const int32_t *none_ptr, const int32_t *none_clause,
                           const srx_doc_filter *base,                           /* host struct or NULL */
                           uint32_t *out_bits,                                   /* device, 16-byte aligned */
                           void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_FIELDS_H */
