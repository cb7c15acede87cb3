/* sparse_rx_rescore.h -- hybrid rescoring: dense scores of caller-given docs and the fusion of two COMPLETED lists.
 *
 * Second header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: the plain fusion gives a doc that only one list returned nothing from the other side, so a fused score depends on
 * how deep the two lists were fetched.  With the sparse scorer of sparse_rx.h ("scores of given docs") and the three
 * dense scorers below, each list can be completed with the OTHER side's exact score of every doc it holds; the scored
 * fusion below then gives every returned doc a fused score that does not depend on the fetch depth.
 *
 * One GPU.  Not covered: a sharded dense corpus, a rescored reciprocal-rank fusion (ranks beyond the fetched depth are
 * unknown) and fused rankings deeper than SRX_MAX_K.
 */
#ifndef SPARSE_RX_RESCORE_H
#define SPARSE_RX_RESCORE_H

#include "sparse_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- dense scores of caller-given docs -------------------------------------------------------------------------------
 *
 * "What does THIS doc score for this query vector": one entry point per form the dense side keeps resident.  Every call
 * is asynchronous on `stream`, allocates nothing, needs no workspace and writes nothing but out_score (f32[nq][m], every
 * word of it).
 *
 * Candidates (the conventions of the sparse scorer):
 *   cand_doc    i32[nq][m], GLOBAL ids; m >= 1, nq * m <= 2^31 - 1.
 *   cand_count  i32[nq] or NULL.  Entries c >= max(cand_count[q], 0) of row q are padding (NULL: no padding).
 *   Padding, and ids whose (int64) cand_doc - doc_base lies outside [0, n_docs), give +0.0f; no corpus byte is read for
 *   them.  Duplicates are legal, each is scored.  There is no score > 0 filter.
 *   The (doc, score, count) triple of a search can be passed as it is.
 *
 * The scores are the bits the searches produce, so a row a dense search returned scores to its own bits
 * (score_offset = 0 for the f32 search):
 *
 *   f32  dim is a multiple of 64, <= 1024.  emb is f32[n_docs][dim], queries f32[nq][dim].  Lane l of 64 holds
 *        p_l = (((+0 + e[l] * q[l]) + e[l + 64] * q[l + 64]) + ...) over the dim / 64 slices in ascending order, every
 *        multiply and every add rounded to fp32 on its own; then for o = 32, 16, 8, 4, 2, 1 every lane takes
 *        a_l = a_l + a_(l xor o); the score is lane 0's value.
 *   u8   the same with e = (float)u8 * corpus_scales[2 d] + corpus_scales[2 d + 1] (two roundings).  corpus is
 *        u8[n_docs][dim], corpus_scales f32[2 n_docs], queries the DE-QUANTIZED f32[nq][dim].
 *   i8   dim is 32, 64, 96, 128, 192, 256, 384, 512, 768 or 1024.  The exact int32 dot product acc, then
 *        (float)(((double)acc * (double)query_scale[q]) * (double)corpus_scale[d]).  packed = 0: corpus is
 *        i8[n_docs][dim]; packed = 1: the fragment order srx_dense_pack_i8 writes -- with T = d / 32, the 16 bytes
 *        [32 s + 16 h, 32 s + 16 h + 16) of row d (s < dim / 32, h in 0 / 1) sit at byte
 *        ((T * (dim / 32) + s) * 64 + (d & 31) + 32 h) * 16.  corpus and queries must be 16-byte aligned.
 *
 * Refused with SRX_ERR_INVALID before anything touches a device: nq < 0; m < 1; nq * m > 2^31 - 1; a dim the form does
 * not take; n_docs outside [1, 2^31 - 2]; packed other than 0 / 1; misaligned i8 corpus / queries; and, with nq > 0, a
 * NULL corpus, scale table, query block, cand_doc or out_score.  nq == 0 returns SRX_OK without a launch.
 */
int srx_dense_score_docs_f32(int32_t device, const float *emb, int64_t n_docs, int32_t dim, const float *queries, int32_t nq,
                             int64_t doc_base, const int32_t *cand_doc, const int32_t *cand_count, int32_t m, float *out_score,
                             void *stream);

int srx_dense_score_docs_u8(int32_t device, const uint8_t *corpus, const float *corpus_scales, int64_t n_docs, int32_t dim,
                            const float *queries, int32_t nq, int64_t doc_base, const int32_t *cand_doc,
                            const int32_t *cand_count, int32_t m, float *out_score, void *stream);

int srx_dense_score_docs_i8(int32_t device, const void *corpus, int32_t packed, const float *corpus_scale, int64_t n_docs,
                            int32_t dim, const int8_t *queries, const float *query_scale, int32_t nq, int64_t doc_base,
                            const int32_t *cand_doc, const int32_t *cand_count, int32_t m, float *out_score, void *stream);

/* ---- fusion of two completed lists (weighted mode) --------------------------------------------------------------------
 *
 * Lists A (a_doc i32[nq][ka], a_score f32[nq][ka], a_count i32[nq]) and B (kb likewise) are ranked top lists over the
 * same doc ids, as for the plain fusion; 1 <= ka, kb, k <= SRX_MAX_K.  New inputs:
 *   a_other  f32[nq][ka]: side B's score of the doc in A's slot.
 *   b_other  f32[nq][kb]: side A's score of the doc in B's slot.
 *
 * Used entries     entry r of list X is used iff r < min(max(x_count[q], 0), kx), x_doc >= 0 and its OWN score is > 0.
 * Normalisers      side X has a normaliser m_X = x_score[q][0] iff entry 0 of list X is used.  A side without a
 *                  normaliser contributes nothing anywhere: neither through its own entries nor through the *_other
 *                  values of the opposite list.
 * Contributions    a score s on side X contributes weight_X * (s / m_X): fp32, each operation rounded on its own (IEEE
 *                  divide, denormals kept).  The own score of a used entry always qualifies; a value from *_other
 *                  contributes iff it is > 0 (NaN, zeros and negative values do not).  The fused score of a used entry
 *                  is the sum of its two contributions, or the one that exists, or +0.
 * Duplicates       a doc that is a used entry of both lists is taken once, from list A: B's entry is dropped whatever
 *                  A's entry fuses to.  Precondition, NOT checked: both lists carry the same two scores for such a
 *                  doc (they do when *_other comes from the exact scorers).  Docs are unique inside a list.
 * Output           as for the plain fusion: the k best fused scores > 0 ordered by (score bits descending, doc
 *                  ascending) in out_doc i32[nq][k] / out_score f32[nq][k], padded with -1 / +0.0; out_count i32[nq].
 *                  The count and every word of both rows are written.
 *
 * Setting *_other to the opposite list's own score where the doc is a used entry of it, and to 0 elsewhere, gives the rows
 * of the plain weighted fusion bit for bit.
 *
 * Refused with SRX_ERR_INVALID before anything touches a device: nq < 0; ka, kb or k out of range; a weight that is
 * negative or not finite; both weights 0; a NULL pointer with nq > 0.  nq == 0 returns SRX_OK without a launch.
 * Asynchronous on `stream`, allocates nothing, needs no workspace.
 */
int srx_fuse_topk_scored(int32_t device, const int32_t *a_doc, const float *a_score, const float *a_other, const int32_t *a_count,
                         int32_t ka, const int32_t *b_doc, const float *b_score, const float *b_other, const int32_t *b_count,
                         int32_t kb, int32_t nq, int32_t k, float weight_a, float weight_b, int32_t *out_doc, float *out_score,
                         int32_t *out_count, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_RESCORE_H */
