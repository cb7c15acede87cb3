/* sparse_rx_maxsim_search.h -- late-interaction SEARCH: the k docs of the whole token store with the best MaxSim score for each
 * query, on the device.
 *
 * Twenty-sixth header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: sparse_rx_maxsim.h only scores GIVEN candidates, and its rerank form stops at 1 024 docs per list.  This header answers
 * "which docs of the corpus have the best MaxSim score for this query": the exhaustive search the multi-vector side lacked, the
 * anchor any later centroid index is pinned to, the recall instrument of a first-stage pool, and -- with a doc filter -- late
 * interaction within a tenant, a date range or a term constraint.  The reference has no multi-vector index: nothing here replaces
 * reference code.
 *
 * ---- the contract, with no tolerance ----------------------------------------------------------------------------------------------
 *
 * The token store (tok_packed, n_tok, dim_pad, tok_ptr, n_docs, doc_base), the queries (q_tok, q_tok_count, nq, tq), the tq /
 * dim_pad limits and the rounding of the query tokens are exactly those of sparse_rx_maxsim.h.  The filter is
 * sparse_rx_filter.h's: rows over the n_docs docs of the store; NULL means no filter, q_filter NULL means row 0 for every query,
 * q_filter[q] == -1 means query q is not filtered.
 *
 * Row q of the output is, word for word, what srx_maxsim_rerank_half writes for query q given the list of ALL docs
 * doc_base .. doc_base + n_docs - 1 that the query's filter row allows, cut to k -- for any n_docs, not only up to 1 024:
 *   - the score of a (query, doc) pair has the bits of srx_maxsim_score_docs_half: one chain of v_mfma_f32_32x32x16_{f16,bf16}
 *     per similarity, k-steps ascending from +0.0f, the query token the A operand and the doc token the B operand; the max is
 *     exact; the ordered fp32 sum runs over the live query tokens;
 *   - a doc with 0 tokens is a result with +0.0f; there is no > 0 filter (scores may be negative);
 *   - the order is (score descending, doc ascending); rows are padded with -1 / +0.0f; out_count[q] = min(k, allowed docs);
 *     every word of out_doc i32[nq][k], out_score f32[nq][k] and out_count i32[nq] is written;
 *   - a query with no live token scores every allowed doc +0.0f: its row holds the first k allowed docs;
 *   - 1 <= k <= SRX_MAX_K (1024);
 *   - the bits of a row do not depend on nq, on the other queries, on the launch geometry, or on the workspace size.
 *
 * ---- workspace, passes, launches ---------------------------------------------------------------------------------------------------
 *
 * The workspace holds the packed, rounded query tokens of the call (nq * ceil32(tq) * dim_pad * 2 bytes, rounded up to 256), the
 * score matrix of one pass -- f32[queries of the pass][ld], ld = n_docs rounded up to 64 -- and, when a score row is split over
 * several workgroups of the selection, their lists of k 64-bit keys; 512 bytes of slack.  A query GROUP is the QG queries whose
 * operands one workgroup of the scan holds in LDS: the largest of 4, 2, 1 with QG * NAB <= 4 (NAB = ceil32(tq) / 32: the
 * accumulator and running-max register sets), QG * NAB * dim_pad / 16 <= 64 (KiB of LDS) and QG < 2 * nq.
 *   minimum    packed queries + min(QG, nq) score rows + slack: the call then runs ceil(nq / QG) passes and ranks every score row
 *              with one workgroup;
 *   preferred  srx_maxsim_search_workspace_bytes(nq, tq, dim_pad, n_docs, k): min(nq, P) score rows, P = the multiple of 4 in
 *              [4, 1024] that keeps the matrix within 1 GiB, plus the key lists of S = clamp(ceil(n_docs / 8192), 1,
 *              max(1, 2048 / rows)) splits per row when S > 1.
 * The call accepts ANY size from the minimum and derives its passes from what it is given: rows = as many as fit, at most the
 * preferred number (whole groups when more than one fits); splits = as many as the rest holds, at most S.  The result does not
 * depend on it.  SRX_ERR_INVALID from the size call for arguments the search refuses.
 *
 * The call allocates nothing, does not synchronise with the host and is asynchronous on `stream`: one launch that packs the
 * query tokens, then per pass one scan, one selection and (split rows) one merge.  nq == 0 returns SRX_OK without a launch.
 *
 * ---- refusals ----------------------------------------------------------------------------------------------------------------------
 *
 * SRX_ERR_INVALID before anything touches a device: a type outside srx_half_type; dim_pad not a multiple of 64 in [64, 1024]; tq
 * outside 1 .. 128 or ceil32(tq) * dim_pad > 32768; k outside 1 .. SRX_MAX_K; n_docs outside [1, 2^31 - 2], n_tok outside
 * [0, 2^31 - 2], a negative doc_base or doc_base + n_docs > 2^31 - 1; nq < 0; a filter with NULL or misaligned (16 bytes) bits or
 * n_filters < 1; with nq > 0 a NULL tok_ptr, q_tok or output, a NULL tok_packed with n_tok > 0, a tok_packed or q_tok that is not
 * 16-byte aligned.  SRX_ERR_NOMEM: a NULL workspace or one below the minimum.
 *
 * Not covered: a centroid (PLAID-style) index, MX or PQ token rows, k > 1 024 or paging, a sharded token store, a top-k fused
 * into the scan.
 */
#ifndef SPARSE_RX_MAXSIM_SEARCH_H
#define SPARSE_RX_MAXSIM_SEARCH_H

#include "sparse_rx.h"
#include "sparse_rx_filter.h"
#include "sparse_rx_maxsim.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t srx_maxsim_search_workspace_bytes(int32_t nq, int32_t tq, int32_t dim_pad, int64_t n_docs, int32_t k);

int srx_maxsim_search_half(int32_t device, int32_t type, const void *tok_packed, int64_t n_tok, int32_t dim_pad,
                           const int32_t *tok_ptr, int64_t n_docs, int64_t doc_base, const float *q_tok,
                           const int32_t *q_tok_count /* may be NULL */, int32_t nq, int32_t tq, int32_t k,
                           const srx_doc_filter *filter /* NULL: none */, int32_t *out_doc, float *out_score, int32_t *out_count,
                           void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_MAXSIM_SEARCH_H */
