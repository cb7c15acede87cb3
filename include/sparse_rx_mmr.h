/* sparse_rx_mmr.h -- diversified top-k: Maximal Marginal Relevance (MMR) selection over result lists, on the device.
 *
 * Sixth header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: every search, the fusion and the scorers end in a ranked (doc, score) list per query.  The docs of a RAG corpus are
 * chunks, and the best chunks of a query are routinely near-copies of each other.  MMR picks k of m candidates greedily,
 * each pick maximising  w_rel * relevance - w_div * (largest similarity to a doc already picked).  The similarities are those
 * of the rows of a resident dense index (f32, or f16 / bf16 in fragment order), so the whole step stays on the device.  The
 * reference has no diversification: like the fusion, the scorers of given docs, the filters and the half-precision index,
 * nothing here replaces reference code.
 *
 * ---- inputs -----------------------------------------------------------------------------------------------------------
 *
 * cand_doc i32[nq][m] GLOBAL ids, cand_rel f32[nq][m], cand_count i32[nq] or NULL: the (doc, score, count) triple of any
 * search or of the fusion goes in unchanged.  1 <= m <= SRX_MMR_MAX_M = 256, 1 <= k <= m.  Position c of query q is LIVE iff
 *   - c < min(max(cand_count[q], 0), m)   (a NULL cand_count means m),
 *   - cand_doc[q][c] - doc_base, computed in 64 bits, is in [0, n_docs),
 *   - cand_rel[q][c] is not NaN.
 * There is no relevance > 0 filter (as in the scorers of given docs).  Preconditions, NOT checked on the device: no doc id
 * twice in one list, finite relevances, finite rows.
 *
 * The f32 form reads emb f32[n_docs][dim] (dim a multiple of 64, at most 1024: rows padded with zeros); the half form reads
 * the packed corpus of sparse_rx_half.h (type of srx_half_type, dim_pad a multiple of 64, at most 1024).
 *
 * ---- similarity -------------------------------------------------------------------------------------------------------
 *
 * G[a][b] of two live positions a, b is, to the bit, the score the scorer of given docs of the same storage (the f32 one of
 * sparse_rx_rescore.h, the half one of sparse_rx_half.h) returns for the query that EQUALS corpus row a and the candidate
 * row b:
 *   f32   lane l of a wave holds columns l, l + 64, ... of both rows; the products are summed in ascending slice order from
 *         +0.0f, each product and each sum rounded on its own, then the 64 lane sums go through the xor butterfly
 *         (distances 32, 16, 8, 4, 2, 1).
 *   half  ONE chain of v_mfma_f32_32x32x16_{f16,bf16} over the k-steps s = 0, 1, ..., dim_pad / 16 - 1 ascending from +0.0f,
 *         row a the A operand and row b the B operand.  The stored 16-bit codes are used as they are (widening them to f32
 *         and rounding again, as the scorer does with its query, is the identity).
 * Every (a, b) is computed in its own orientation: nothing here assumes that G is bitwise symmetric, and nothing is
 * mirrored.
 *
 * sim_mode SRX_MMR_DOT:     S(a, b) = G[a][b].
 * sim_mode SRX_MMR_COSINE:  n[a] = fl(sqrt(G[a][a]))  (correctly rounded IEEE square root),  d = fl(n[a] * n[b]),
 *                           S(a, b) = d > 0 ? fl(G[a][b] / d) : +0.0f  (IEEE divide).
 *
 * ---- selection --------------------------------------------------------------------------------------------------------
 *
 * fp32, every operation rounded on its own (no fused multiply-add).
 *   step t = 0:   v(c) = fl(w_rel * rel[c])
 *   step t >= 1:  pen[c] = the largest S(c, s) over the docs s picked so far (candidate first, picked doc second),
 *                 v(c) = fl(fl(w_rel * rel[c]) - fl(w_div * pen[c]))
 * Each step picks the live, unpicked position with the greatest v; ties (float ==) go to the lowest position.  Selection
 * stops after k picks or when no live position is left.
 *
 * Row q of the outputs, padded with -1 / +0.0f:
 *   out_doc[q][t]   i32[nq][k]  the doc picked at step t -- SELECTION order, not relevance order
 *   out_rel[q][t]   f32[nq][k]  its relevance exactly as given
 *   out_mmr[q][t]   f32[nq][k]  v at the step it was picked (may be NULL)
 *   out_count[q]    i32[nq]     min(k, live positions)
 * out_sim (may be NULL) f32[nq][m][m] receives G; entries with a dead row or column are +0.0f.  It is the Gram stage's own
 * output buffer, not a second computation.  Every word of every output row and every count is written.
 *
 * ---- workspace, launches ----------------------------------------------------------------------------------------------
 *
 * The workspace holds G of the call: the size query returns nq * m * m * 4 bytes plus alignment slack (SRX_ERR_INVALID for
 * nq < 0 or m outside 1 .. 256).  It is required even when out_sim is given: G is then written to out_sim, the workspace
 * may be that same buffer, and nq * m * m * 4 bytes are enough.  The calls allocate nothing and are asynchronous on `stream`:
 * one Gram launch and one selection launch.  nq == 0 returns SRX_OK without a launch.
 *
 * ---- refusals ---------------------------------------------------------------------------------------------------------
 *
 * SRX_ERR_INVALID before anything touches a device: m outside 1 .. 256 or k outside 1 .. m; a sim_mode outside srx_mmr_sim;
 * a type outside srx_half_type; a weight that is negative or not finite, or both weights 0; dim / dim_pad not a multiple of 64
 * in [64, 1024]; n_docs outside [1, 2^31 - 2] or a negative doc_base; nq < 0 or nq * m > 2^31 - 1; with nq > 0 a NULL corpus, cand_doc, cand_rel,
 * out_doc, out_rel or out_count, and (half form) a corpus that is not 16-byte aligned.  SRX_ERR_NOMEM: a NULL or too small
 * workspace.
 */
#ifndef SPARSE_RX_MMR_H
#define SPARSE_RX_MMR_H

#include "sparse_rx.h"
#include "sparse_rx_half.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRX_MMR_MAX_M 256

typedef enum { SRX_MMR_DOT = 0, SRX_MMR_COSINE = 1 } srx_mmr_sim;

int64_t srx_mmr_workspace_bytes(int32_t nq, int32_t m);

int srx_mmr_select_f32(int32_t device, const float *emb, int64_t n_docs, int32_t dim, int64_t doc_base,
                       const int32_t *cand_doc, const float *cand_rel, const int32_t *cand_count /* may be NULL */, int32_t nq, int32_t m,
                       int32_t k, int32_t sim_mode, float w_rel, float w_div,
                       int32_t *out_doc, float *out_rel, float *out_mmr /* may be NULL */, int32_t *out_count,
                       float *out_sim /* may be NULL: f32[nq][m][m] */, void *workspace, int64_t workspace_bytes, void *stream);

int srx_mmr_select_half(int32_t device, int32_t type, const void *corpus_packed, int64_t n_docs, int32_t dim_pad, int64_t doc_base,
                        const int32_t *cand_doc, const float *cand_rel, const int32_t *cand_count /* may be NULL */, int32_t nq, int32_t m,
                        int32_t k, int32_t sim_mode, float w_rel, float w_div,
                        int32_t *out_doc, float *out_rel, float *out_mmr /* may be NULL */, int32_t *out_count,
                        float *out_sim /* may be NULL: f32[nq][m][m] */, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_MMR_H */
