/* sparse_rx_terms.h -- term constraints: filter rows built on the device from the posting lists of an index.
 *
 * Seventh header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: a filter row (sparse_rx_filter.h) restricts a sparse, dense or hybrid search to a doc set, but the only ways to make one
 * are a host mask and a list of doc ids.  "Docs that contain term t" is the question the posting lists answer, and they are
 * resident: this header turns (must all / must any / must none) term lists into filter rows without a host walk of the
 * corpus -- Lucene's bool query (must, should with a minimum match of 1, must_not) as a doc set.  The rows go to every
 * filtered search as they are, so they also give keyword-constrained vector and hybrid search.  The reference has no filters:
 * nothing here replaces reference code.
 *
 * ---- the contract -----------------------------------------------------------------------------------------------------
 *
 * Lists        three ragged lists of term ids per output row, each a device CSR: ptr i32[n_rows + 1] (ptr[0] = 0, ascending)
 *              and term i32[ptr[n_rows]].  A list is absent for every row when BOTH its pointers are NULL.
 * Row r allows local doc d (0 <= d < n_docs) iff all of
 *                base(r, d)            the base filter's row q_filter[r] allows d (q_filter NULL: row 0; -1: every doc; a NULL
 *                                      base: every doc) -- base->q_filter is read per OUTPUT row, i32[n_rows];
 *                all[r]                d has every term of the list;
 *                any[r]                the list is empty, or d has at least one of its terms;
 *                none[r]               d has no term of the list.
 * "d has t"    the index STORES a posting of term t for doc d: a real id, not a sentinel, whatever its value.  The build
 *              (srx_build_blocks and what feeds it) never drops an input entry: an explicitly stored zero is a posting, and
 *              duplicate (doc, term) entries are summed into ONE posting that stays even when the sum is zero.  So the rule
 *              is about the entries of the matrix the index was built from, not about non-zero values.
 * Term ids     -1 is legal in every list and means "a term no doc has" (an out-of-vocabulary word): in `all` it makes the
 *              row empty, in `any` it contributes nothing but the list counts as non-empty, in `none` it has no effect.  Any
 *              other id outside [0, vocab) is a PRECONDITION violation, not checked on the device.  Duplicates are legal; a
 *              term in both `all` and `none` gives an empty row.
 * Output       every word of every row is written: out_bits u32[n_rows][words], words = srx_filter_words of n_docs; bits at
 *              or above n_docs and the padding words are 0 (the row contract of srx_filter_fill).  out_bits must not overlap
 *              base->bits.
 * The call is asynchronous on `stream`, allocates nothing, needs no workspace and uses no global atomics.  It reads whichever
 * copy of the postings the descriptor holds (post16 when given, else post) and never reads a value, so both value types cost the
 * same.
 *
 * Refused with SRX_ERR_INVALID before anything touches a device: what srx_score_docs refuses of a descriptor (NULL, val_type,
 * n_docs / vocab, tile_log2, n_tiles, unit_tiles, neither post nor post16, a compact copy with units of more than 49152 docs,
 * NULL term_ptr / tile_skip / idf); n_rows < 0; one pointer of a ptr / term pair NULL without the other; a NULL or
 * misaligned (16 bytes) out_bits; a base that srx_search_filtered would refuse (NULL or misaligned bits, n_filters < 1).
 * n_rows == 0 returns SRX_OK without a launch.
 *
 * srx_filter_from_terms_bytes   host only: the size of out_bits, n_rows * words * 4 bytes; SRX_ERR_INVALID for
 *              n_rows < 0, n_docs outside [1, 2^31 - 2] or a product that does not fit int64.
 *
 * Not covered: phrase constraints (the index has no positions), a sharded index (rows are shard-local, as every filter's).
 */
#ifndef SPARSE_RX_TERMS_H
#define SPARSE_RX_TERMS_H

#include "sparse_rx_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t srx_filter_from_terms_bytes(int64_t n_rows, int64_t n_docs);

int srx_filter_from_terms(const srx_index_desc *h_desc, int32_t n_rows,
                          const int32_t *all_ptr, const int32_t *all_term,   /* device CSR; both NULL = no such list */
                          const int32_t *any_ptr, const int32_t *any_term,
                          const int32_t *none_ptr, const int32_t *none_term,
                          const srx_doc_filter *base,                        /* host struct or NULL */
                          uint32_t *out_bits,                                /* device, 16-byte aligned */
                          void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_TERMS_H */
