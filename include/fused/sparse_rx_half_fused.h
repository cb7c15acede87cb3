/* sparse_rx_half_fused.h -- the half-precision dense search with the top-k screen fused into the GEMM.
 *
 * Twenty-third header of libsparse_rx.so (same library, same conventions as sparse_rx.h).  It adds a second route to the
 * search of sparse_rx_half.h over the SAME packed corpus: srx_dense_search_half writes an nq x n_docs fp32 score matrix and
 * reads it back to rank it; this call never forms that matrix.  The reference has no half-precision index: nothing here
 * replaces reference code.
 *
 * ---- contract -----------------------------------------------------------------------------------------------------------
 *
 * srx_dense_search_half_fused takes exactly the parameters of srx_dense_search_half.  For every argument list that call
 * accepts, this one writes the same words: out_doc, out_score and out_count, padding included, with or without a filter,
 * for any q_filter, score_offset, doc_base and k in 1 .. SRX_MAX_K.  Why that holds:
 *   - the ranking rule is total: ranked value fl32(score + score_offset) descending, doc ascending, only values > 0, a
 *     filtered query only over the docs of its row.  The top k of a set under a total order is one list, however it is found;
 *   - the score bits of a (query, doc) pair do not depend on which kernel produced them (the promise of sparse_rx_half.h:
 *     one ascending chain of v_mfma_f32_32x32x16_{f16,bf16} per output element, each element from its own row and column
 *     operands only).  All kernels here run that chain.
 * Refusals are those of srx_dense_search_half, checked in the same order; SRX_ERR_NOMEM is judged against
 * srx_dense_half_fused_workspace_bytes.  The entry point always takes the fused path: there is no corpus-size switch back
 * to the matrix route.  No host synchronisation: the overflow state stays on the device.
 *
 * ---- how ----------------------------------------------------------------------------------------------------------------
 *
 * Queries go in passes of up to SRX_HALF_FUSED_PASS = 1024, whatever n_docs is.  Per pass:
 *   1. threshold.  The first S docs (the sample; S below) are scored into an [queries][S] matrix and ranked by the kernels of
 *      srx_dense_search_half, with the filter row, q_filter and score_offset applied.  tau[q] = the bit pattern of the k-th
 *      best ranked value of the sample when the sample holds k results of query q, else 0 ("keep every result").  Because
 *      the sample is ranked under the query's filter, tau is a lower bound of the k-th best ALLOWED doc's value: every member
 *      of the final top k has ranked bits >= tau[q].  (Positive floats order as their bit patterns.)
 *   2. fused GEMM over ALL docs: the 128 x 128 tile of srx_dense_search_half; instead of storing the tile a lane forms
 *      x = fl32(acc + score_offset) and keeps it iff x > 0 and bits(x) >= tau[q]; only then is the filter bit fetched.  A
 *      survivor takes a slot of its query's candidate buffer with one vector atomic add and writes (doc, bits).  A slot at
 *      or beyond SRX_HALF_FUSED_CAP sets the query's overflow flag instead.
 *   3. rank.  A query that did not overflow has its buffer folded into an exact top-k list and ranked (buffer order is not
 *      deterministic; the result is, the rule being total).
 *   4. exact fallback for overflowed queries only (all-tied or filter-starved rows): the query against its doc range in
 *      32-row tiles through the chain of srx_dense_score_docs_half, folded directly -- no matrix.  Slow, exact, and not
 *      launched into work unless some query overflowed.
 *
 * ---- constants ----------------------------------------------------------------------------------------------------------
 *
 * SRX_HALF_FUSED_CAP       entries of a query's candidate buffer (8 bytes each).
 * SRX_HALF_FUSED_MIN_DOCS  below this many docs there is no sample (S = 0, tau = 0): the buffers hold every result, and
 *                          since MIN_DOCS <= CAP they cannot overflow.
 * Sample rule (the INT8 search's, dense.hip): S = 0 if n_docs < MIN_DOCS; else
 *     S = max(ceil(3 k n_docs / CAP), clamp(164 k, 4096, 16384)) rounded up to a multiple of 128, and S = 0 if 4 S > n_docs.
 * About k n_docs / S docs per query pass a threshold taken from S docs: the first term aims at CAP / 3 survivors, the floor
 * keeps the sample pass (which does go through a matrix) short.  CAP and the rule are the INT8 search's values; profiles/
 * half_fused.log records the survivors per query and the share of overflowed queries they give on the half index.
 *
 * Workspace, each term rounded up to 256 bytes, plus 256, with qb = min(nq, 1024):
 *     packed queries   ceil(qb / 128) * 128 * 2048
 *     sample matrix    qb * S * 4
 *     lists            3 terms: qb * L * k * 4 (docs), the same (scores), qb * L * 4 (counts), L = fallback splits =
 *                      clamp(ceil(n_docs / 32) / 64, 1, min(4096 / k, 64))
 *     tau, counters    qb * 4;  (qb * 32 + qb + 1) * 4 (a 128-byte line per buffer counter, the overflow flags, any-overflow)
 *     buffers          2 terms of qb * CAP * 4 (docs, bits)
 * The score matrix of the corpus (qb * n_docs * 4) is gone.  The only term in qb and n_docs together is the sample's, and it
 * is the matrix scaled by S / n_docs = max(3 k / CAP, floor / n_docs): 19 MB for 1024 queries over 10 M docs at k = 10 where
 * srx_dense_search_half asks for 3.8 GB; 1.9 GB at k = 1000, which a second threshold round (not built) would cut.
 * THE FUSED WORKSPACE CAN BE THE LARGER ONE.  A pass always holds up to 1024 queries: a full pass needs about 0.5 GiB of buffers
 * plus 0.1875 k n_docs bytes of sample matrix.  The matrix route needs 4096 n_docs bytes for a full pass but shrinks its pass
 * to keep that within 4 GiB (128 bytes per doc beyond 2^25 docs).  So for 1024 queries the fused workspace is the larger one
 * below about 130 k docs (the buffers outweigh the matrix), and at large k over large corpora: at k = 1000 from about 20 M docs
 * on (k n_docs > 2 * 10^10; 187.5 bytes per doc against 128).  At k = 100 (18.75 bytes per doc) it stays the smaller one at every
 * size above 130 k docs.  The workspace call returns the size; the caller decides, or sends fewer queries per call.
 *
 * Not covered: a second, tighter threshold round; a fused screen for the MX / PQ / IVF scans; a sharded
 * dense corpus; HybridRetriever.
 */
#ifndef SPARSE_RX_HALF_FUSED_H
#define SPARSE_RX_HALF_FUSED_H

#include "sparse_rx_half.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRX_HALF_FUSED_CAP 65536
#define SRX_HALF_FUSED_MIN_DOCS 65536
#define SRX_HALF_FUSED_PASS 1024

int64_t srx_dense_half_fused_workspace_bytes(int32_t nq, int64_t n_docs, int32_t k);

int srx_dense_search_half_fused(int32_t device, int32_t type, const void *corpus_packed, int64_t n_docs, int32_t dim_pad,
                                const float *queries, int32_t nq, int32_t k, int64_t doc_base, const srx_doc_filter *filter /* NULL: none */,
                                int32_t *out_doc, float *out_score, int32_t *out_count, void *workspace, int64_t workspace_bytes,
                                void *stream, float score_offset);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_HALF_FUSED_H */
