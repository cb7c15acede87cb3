/* sparse_rx_maxsim.h -- late-interaction reranking: MaxSim (ColBERT-style) scores of given (query, doc) pairs over
 * half-precision token rows, and the top-k of a candidate list by them, on the device.
 *
 * Eighth header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: a retrieve-then-refine pipeline first-stage retrieves with BM25 and / or one vector per doc, fuses the lists, and
 * then reorders the best 100 .. 1000 candidates with a stronger scorer.  Late interaction keeps SEVERAL vectors per doc (one
 * per token or passage) and scores a pair as the sum, over the query's token vectors, of the largest similarity to any of
 * the doc's token vectors.  It is a batched, gather-heavy, matrix-multiply-shaped scorer of GIVEN pairs: the shape of
 * srx_dense_score_docs_half with many rows per doc.  The reference has no reranker, no multi-vector index and no late
 * interaction: like the fusion, the scorers of given docs, the filters, the half-precision index and the MMR selection,
 * nothing here replaces reference code.
 *
 * ---- token store ------------------------------------------------------------------------------------------------------
 *
 * The token vectors of ALL docs are the rows of ONE packed half corpus, exactly as sparse_rx_half.h lays it out: n_tok rows,
 * dim_pad columns (a multiple of 64 in [64, 1024]), type of srx_half_type, 16-byte aligned, written by
 * srx_dense_convert_half (there is no other conversion).  tok_ptr i32[n_docs + 1] holds the token row range of each doc: doc
 * d owns token rows tok_ptr[d] .. tok_ptr[d + 1] - 1; it is non-decreasing with tok_ptr[0] == 0 and
 * tok_ptr[n_docs] == n_tok <= 2^31 - 2.  A doc may have 0 tokens; a doc's rows start at any row, not at tile boundaries.
 * (The kernels clamp every range to [0, n_tok): a tok_ptr that breaks the rules gives wrong scores, never a read outside the
 * store.)
 *
 * ---- queries ----------------------------------------------------------------------------------------------------------
 *
 * q_tok f32[nq][tq][dim_pad] (columns dim .. dim_pad - 1 zero), 16-byte aligned.  q_tok_count i32[nq] or NULL: query token
 * i of query q is LIVE iff i < min(max(q_tok_count[q], 0), tq) (NULL means tq).  The query tokens are rounded to the corpus
 * type with the corpus's rounding (nearest even), as the half search rounds its queries.
 * 1 <= tq <= SRX_MAXSIM_MAX_QT = 128 and ceil32(tq) * dim_pad <= 32768 (ceil32: rounded up to a multiple of 32): 32 query
 * tokens at dim_pad 1024, 64 at 512, 128 at 256 or below -- the query's operand fragments then fit 64 KiB of LDS.
 *
 * ---- score ------------------------------------------------------------------------------------------------------------
 *
 * sim(i, j), the similarity of live query token i and token row j of the doc, is, to the bit, what
 * srx_dense_score_docs_half returns for the query that is that f32 query token and the candidate that is that token row, in
 * a half corpus holding the token rows: ONE chain of v_mfma_f32_32x32x16_{f16,bf16} over the k-steps s = 0, 1, ...,
 * dim_pad / 16 - 1 ascending from +0.0f, the query token the A operand and the doc token the B operand; no split-K.  The
 * arithmetic inside one instruction stays the hardware's and is not restated.
 *   M(i)  = max over the doc's token rows j of sim(i, j)                       (the max is exact)
 *   score = (((+0.0f + M(i0)) + M(i1)) + ...) over the LIVE query tokens i0 < i1 < ... in ascending order, each add rounded
 *           on its own (fp32, no fused operation); dead query tokens are skipped.
 * A doc with 0 tokens, or a query with no live token, scores +0.0f.  Rows of other docs and the zero rows that pad a tile
 * never take part in the max (a doc whose similarities are all negative scores the sum of the least negative ones, not 0).
 * Preconditions, NOT checked on the device: finite token rows (srx_dense_convert_half zeroes non-finite rows and raises its
 * flag) and finite query tokens.  The bits of a (query, doc) score do not depend on nq, on the other queries and their
 * counts, on m, or on the position in the list.
 *
 * ---- srx_maxsim_score_docs_half ---------------------------------------------------------------------------------------
 *
 * The contract of srx_dense_score_docs_half: cand_doc i32[nq][m] GLOBAL ids, cand_count i32[nq] or NULL, out_score
 * f32[nq][m] with every word written; padding (-1, entries at or beyond cand_count[q]) and ids outside
 * [doc_base, doc_base + n_docs) give +0.0f; no > 0 filter; duplicates are legal; m is limited only by nq * m <= 2^31 - 1.
 *
 * ---- srx_maxsim_rerank_half -------------------------------------------------------------------------------------------
 *
 * 1 <= m <= SRX_MAX_K (1024), 1 <= k <= m.  Scores as above, then ranks the LIVE positions (c < min(max(cand_count[q], 0), m)
 * and id in [doc_base, doc_base + n_docs); a doc with 0 tokens is live with +0.0f) by (score descending, doc ascending).
 * There is no > 0 filter: MaxSim scores may be negative.  Row q of out_doc i32[nq][k] / out_score f32[nq][k] is padded with
 * -1 / +0.0f; out_count[q] = min(k, live positions).  Every word of every output row and count is written.  Precondition:
 * no doc id twice in one list.
 *
 * ---- workspace, launches ----------------------------------------------------------------------------------------------
 *
 * srx_maxsim_workspace_bytes(nq, tq, dim_pad, m): the packed, rounded query tokens of the call (nq * ceil32(tq) * dim_pad * 2
 * bytes) and, for m >= 1, the f32[nq][m] score matrix of the rerank form, plus alignment slack.  m == 0 gives the size the
 * scorer form needs (it has no matrix; a size queried with m >= 1 serves it as well).  SRX_ERR_INVALID for nq < 0, tq or
 * dim_pad outside the limits above, m outside 0 .. SRX_MAX_K, nq * m > 2^31 - 1.  The calls allocate nothing and are
 * asynchronous on `stream`: one launch that packs the query tokens, one that scores and (rerank) one that ranks.  nq == 0
 * returns SRX_OK without a launch.
 *
 * ---- refusals ---------------------------------------------------------------------------------------------------------
 *
 * SRX_ERR_INVALID before anything touches a device: a type outside srx_half_type; dim_pad not a multiple of 64 in
 * [64, 1024]; tq outside 1 .. 128 or ceil32(tq) * dim_pad > 32768; m < 1 (rerank: m outside 1 .. 1024, k outside 1 .. m);
 * n_docs outside [1, 2^31 - 2], n_tok outside [0, 2^31 - 2], a negative doc_base; nq < 0 or nq * m > 2^31 - 1; with nq > 0
 * a NULL tok_ptr, q_tok, cand_doc or output, a NULL tok_packed with n_tok > 0, a tok_packed or q_tok that is not 16-byte
 * aligned.  SRX_ERR_NOMEM: a NULL or too small workspace.
 */
#ifndef SPARSE_RX_MAXSIM_H
#define SPARSE_RX_MAXSIM_H

#include "sparse_rx.h"
#include "sparse_rx_half.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRX_MAXSIM_MAX_QT 128

int64_t srx_maxsim_workspace_bytes(int32_t nq, int32_t tq, int32_t dim_pad, int32_t m);

int srx_maxsim_score_docs_half(int32_t device, int32_t type, const void *tok_packed, int64_t n_tok, int32_t dim_pad,
                               const int32_t *tok_ptr, int64_t n_docs, int64_t doc_base, const float *q_tok,
                               const int32_t *q_tok_count /* may be NULL */, int32_t nq, int32_t tq, const int32_t *cand_doc,
                               const int32_t *cand_count /* may be NULL */, int32_t m, float *out_score, void *workspace,
                               int64_t workspace_bytes, void *stream);

int srx_maxsim_rerank_half(int32_t device, int32_t type, const void *tok_packed, int64_t n_tok, int32_t dim_pad,
                           const int32_t *tok_ptr, int64_t n_docs, int64_t doc_base, const float *q_tok,
                           const int32_t *q_tok_count /* may be NULL */, int32_t nq, int32_t tq, const int32_t *cand_doc,
                           const int32_t *cand_count /* may be NULL */, int32_t m, int32_t k, int32_t *out_doc, float *out_score,
                           int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_MAXSIM_H */
