/* sparse_rx_filter.h -- filtered search: sparse and dense retrieval restricted to a set of docs.
 *
 * Fourth header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: every search of sparse_rx.h ranks the whole corpus.  Tombstones, a tenant's docs, the result of a metadata
 * predicate and "not the ones already shown" all need the top k OF A SET; removing rows from a returned list is not that
 * (a top-100 list with 60 rows removed is not the top 100 of the allowed docs).  The reference has no filters at all:
 * like the fusion and the scorers of given docs, nothing here replaces reference code.
 *
 * ---- the contract -----------------------------------------------------------------------------------------------------
 *
 * Filter row   a bitmap over the SHARD-LOCAL rows of an index: doc d (0 <= d < n_docs) is allowed iff bit d & 31 of word
 *              d >> 5 is set.  A row is srx_filter_words(n_docs) 32-bit words long: ceil(n_docs / 32) rounded up to a
 *              multiple of 4, so every row of an array of rows is 16-byte aligned when the array is.  Bits at or above
 *              n_docs are never read as docs.
 * Filter       n_filters >= 1 such rows in one device array `bits` (row r at bits + r * words), plus an optional device
 *              array q_filter i32[nq] that picks a row per query:
 *                q_filter == NULL    every query uses row 0;
 *                q_filter[q] == -1   query q is not filtered;
 *                a value outside [-1, n_filters) is a PRECONDITION violation, not checked on the device.
 * Result       a filtered search returns, for query q, what the unfiltered search returns at unlimited depth with the
 *              rows of disallowed docs removed, cut to k: same arithmetic, same fp32 score bits, same (score descending,
 *              doc ascending) order, same score > 0 rule, same -1 / +0.0 padding; every word of every row and every
 *              count is written.  A filter that allows nothing gives count 0.
 * Ids          filter bits speak of shard-local rows; returned ids and the after_doc bound stay GLOBAL (doc_base + row).
 * The bitmap is only read by a search; it must not be written while one that uses it is in flight.
 *
 * Not covered: the INT8 dense search (its fused screen derives thresholds from a sample of ALL docs), a sharded index.
 */
#ifndef SPARSE_RX_FILTER_H
#define SPARSE_RX_FILTER_H

#include "sparse_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct srx_doc_filter {
    const uint32_t *bits;    /* device, u32[n_filters][words], 16-byte aligned */
    int32_t n_filters;       /* >= 1 */
    const int32_t *q_filter; /* device, i32[nq], or NULL */
} srx_doc_filter;

/* ---- building filter rows ---------------------------------------------------------------------------------------------
 *
 * srx_filter_words   host only: words per row for n_docs docs; SRX_ERR_INVALID for n_docs outside [1, 2^31 - 2].
 * srx_filter_fill    every doc bit of every row becomes `value` (0 / 1); the bits of the last word at or above n_docs
 *                    and the padding words become 0.
 * srx_filter_set_docs  sets (value 1) or clears (value 0) the bits of the n listed GLOBAL ids doc i32[n] in ONE row
 *                    (row_bits = bits + r * words).  Ids outside [doc_base, doc_base + n_docs), -1 included, are ignored,
 *                    so a result row of either search engine can be passed as it is.  Duplicates are legal.  One launch
 *                    of vector atomics; concurrent calls on the same row are safe.
 * srx_filter_count   out_count[r] = allowed docs of row r (i32[n_filters], every word written).
 *
 * The three device calls are asynchronous on `stream`, allocate nothing and need no workspace.  Refused with
 * SRX_ERR_INVALID before anything touches a device: n_docs outside [1, 2^31 - 2]; n_filters < 1; value other than 0 / 1;
 * n < 0; a doc_base that is negative or with doc_base + n_docs >= 2^31 - 1; a NULL or misaligned (16 bytes) bits / row_bits;
 * a NULL doc with n > 0; a NULL out_count.  n == 0 returns SRX_OK without a launch.
 */
int64_t srx_filter_words(int64_t n_docs);

int srx_filter_fill(int32_t device, uint32_t *bits, int32_t n_filters, int64_t n_docs, int32_t value, void *stream);

int srx_filter_set_docs(int32_t device, uint32_t *row_bits, int64_t n_docs, int64_t doc_base, const int32_t *doc, int64_t n,
                        int32_t value, void *stream);

int srx_filter_count(int32_t device, const uint32_t *bits, int32_t n_filters, int64_t n_docs, int32_t *out_count, void *stream);

/* ---- filtered sparse search -------------------------------------------------------------------------------------------
 *
 * The arguments of the plain / packed search of sparse_rx.h, plus the filter (a HOST struct, read during the call; its
 * rows are over ix's n_docs local rows) and the bound row of the search-after call: after_doc i32[nq] GLOBAL ids and
 * after_score f32[nq], both NULL (no bound) or both given.  Given, they page a filtered ranking exactly as search-after
 * pages a plain one: only allowed docs ranked strictly after (after_score[q], after_doc[q]) are returned.  The workspace
 * is the plain search's (srx_search_workspace_bytes).
 *
 * Every candidate is tested where the tier-2 kernel forms it; the per-term score bounds are not used (they speak of the k
 * best of ALL docs: a threshold derived from a disallowed doc would cut allowed ones), tier 1 scores nothing.
 *
 * Refused with SRX_ERR_INVALID before anything touches a device, in addition to the plain search's refusals: a NULL
 * filter; NULL or misaligned (16 bytes) filter->bits; n_filters < 1; only one of after_doc / after_score.  nq == 0
 * returns SRX_OK without a launch.
 */
int srx_search_filtered(srx_index *ix, const int32_t *q_ptr, const int32_t *q_term, const float *q_weight, int32_t nq, int32_t k,
                        const srx_doc_filter *filter, const int32_t *after_doc, const float *after_score, int32_t *out_doc,
                        float *out_score, int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream);

int srx_search_filtered_packed(srx_index *ix, const int32_t *q_ptr, const int32_t *q_term, const float *q_weight, int32_t nq,
                               int32_t k, const srx_doc_filter *filter, const int32_t *after_doc, const float *after_score,
                               int32_t *out_packed, void *workspace, int64_t workspace_bytes, void *stream);

/* ---- filtered dense search (f32 and uint8 rows) -----------------------------------------------------------------------
 *
 * The arguments of the unfiltered calls of sparse_rx.h plus the filter (rows over the n_docs rows of emb / corpus); the
 * scores are computed as there, column d of a query's score row is ranked iff its bit is set.  The workspace is
 * srx_dense_f32_workspace_bytes.  Refusals: the unfiltered call's, and the filter's as above.
 */
int srx_dense_search_f32_filtered(int32_t device, const float *emb, int64_t n_docs, int32_t dim, const float *queries, int32_t nq,
                                  int32_t k, int64_t doc_base, const srx_doc_filter *filter, int32_t *out_doc, float *out_score,
                                  int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream, float score_offset);

int srx_dense_search_u8_filtered(int32_t device, const uint8_t *corpus, const float *corpus_scales, int64_t n_docs, int32_t dim,
                                 const float *queries, int32_t nq, int32_t k, int64_t doc_base, const srx_doc_filter *filter,
                                 int32_t *out_doc, float *out_score, int32_t *out_count, void *workspace, int64_t workspace_bytes,
                                 void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_FILTER_H */
