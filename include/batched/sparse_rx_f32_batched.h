/* sparse_rx_f32_batched.h -- the f32 dense search for query batches: an fp32 MFMA screen, then exact rescoring.
 *
 * Twenty-fourth header of libsparse_rx.so (same library, same conventions as sparse_rx.h).  It adds a second route to
 * srx_dense_search_f32 / srx_dense_search_f32_filtered over the SAME row-major f32 matrix: those stream the matrix from HBM
 * once per four queries; this call reads it once per pass of up to 1024 queries (plus a gathered read per surviving pair).
 * The reference has no batched search: nothing here replaces reference code.
 *
 * ---- contract -----------------------------------------------------------------------------------------------------------
 *
 * srx_dense_search_f32_batched takes exactly the parameters of srx_dense_search_f32_filtered; a NULL filter means "no filter"
 * (the words of srx_dense_search_f32).  For every argument list those calls accept, this one writes the same words: out_doc,
 * out_score and out_count, padding included, for any q_filter, score_offset, doc_base and k in 1 .. SRX_MAX_K.  There is no
 * tolerance.  Why that holds:
 *   - the ranking rule is total: ranked value fl32(score + score_offset) descending, doc ascending, only values > 0, a filtered
 *     query only over the docs of its row.  The top k of a set under a total order is one list, however it is found;
 *   - every score that reaches a list is computed by the arithmetic of srx_dense_f32_scores_kernel and
 *     srx_dense_score_docs_f32 (lane l sums the products of columns l, l + 64, ... in ascending order from +0, unfused; the
 *     fixed xor butterfly 32, 16, .. 1; one rounded addition of score_offset).  The MFMA values never reach an output: they
 *     only decide which (query, doc) pairs are rescored;
 *   - a pair is dropped by the screen only when its exact ranked value is provably below the query's threshold (margin below).
 * Refusals are those of srx_dense_search_f32_filtered, checked in the same order (a non-NULL filter first); SRX_ERR_NOMEM is
 * judged against srx_dense_f32_batched_workspace_bytes.  The entry point always takes the batched path: there is no size
 * switch.  No host synchronisation: the overflow state stays on the device.  Non-finite inputs: a NaN screen value is kept and
 * the exact arithmetic decides; nothing more is promised.
 *
 * ---- margin -------------------------------------------------------------------------------------------------------------
 *
 * Let u = 2^-24, n = dim, gamma = n u / (1 - n u).  Any fp32 evaluation of sum q_i d_i whose products and partial sums are each
 * rounded to nearest -- fused or not, in any order -- differs from the real sum by at most gamma * sum |q_i d_i| (Higham,
 * Accuracy and Stability, section 3.1: every term passes through at most n roundings).  Two such evaluations therefore differ by
 * at most 2 gamma sum |q_i d_i| <= 2 gamma ||q||_2 ||d||_2 (Cauchy-Schwarz) <= 2 gamma ||q||_2 R, R an upper bound of the largest
 * row norm.  The exact chain is one such evaluation.  THE PREMISE for v_mfma_f32_32x32x2_f32 -- that its internal steps round to
 * nearest -- is not documented; it was measured (tools/f32_mfma_probe.hip, profiles/f32_batched.log): the largest
 * |MFMA chain - float64| / sum |q_i d_i| over Gaussian rows, rows with blocks of very different magnitude and cancelling rows,
 * dims 64 .. 1024, is SRX_F32_BATCHED_MEASURED_RATIO * gamma.  The margin takes c = max(2, 4 * that ratio) = SRX_F32_BATCHED_C:
 *
 *     m_q = c * 2 gamma ||q||_2 R * (1 + 2^-20)  +  2^-126 (2 n + ||q||_1 + sqrt(n) R)
 *
 * ||q|| is summed in fp64 per query; R = sqrt(largest fp32 sum of squares of a row) * (1 + 2^-9), computed on the device by one
 * streaming pass per CALL (the parameter list has no place for a cached value; the pass costs one read of the matrix, what the
 * matvec route pays per four queries).  The second term covers inputs, products and sums flushed to zero below 2^-126.
 * The screen's own arithmetic is done once per query in fp64 and rounded DOWN to fp32, so the kernel compares and nothing else:
 *     bound_q = rd32( pred(tau_q) - score_offset - m_q - 2^-48 (|score_offset| + tau_q) )            (tau_q = 0: pred(0) := 0)
 * and a pair is dropped iff x~ < bound_q (a NaN is kept).  Chain: x~ < bound_q  =>  s <= x~ + m_q < pred(tau) - offset - (fp64
 * rounding of the two subtractions, <= 2^-51 (|offset| + tau))  =>  s + offset < pred(tau) in real numbers  =>
 * fl32(s + offset) <= pred(tau) < tau.  With tau = 0 the same chain gives s + offset < 0: not a result.
 *
 * ---- how ----------------------------------------------------------------------------------------------------------------
 *
 * Queries go in passes of up to SRX_F32_BATCHED_PASS = 1024.  Per pass:
 *   1. threshold.  The first S docs (the sample; S below) go through the MFMA kernel into an [queries][S] matrix.  A sample doc
 *      allowed by the query's filter row counts with y = rd32(x~ + score_offset - m_q - 2^-48 (|score_offset| + |x~|)) if y > 0:
 *      y under-estimates the exact ranked value of the same doc.  tau[q] = the k-th best y when there are k, else 0 ("keep every
 *      positive candidate").  tau is a lower bound of the k-th best ranked value among the allowed docs.
 *   2. screen GEMM over ALL docs (the hot kernel): queries x docs by v_mfma_f32_32x32x2_f32 from the f32 rows as they lie in
 *      memory.  A workgroup of four waves owns a 128 x 128 tile, a wave 64 x 64 (four 32 x 32 accumulators).  Both operands pass
 *      through LDS in chunks of 32 columns, two buffers, the loads of chunk c + 1 in flight during the MFMAs of chunk c.  An LDS
 *      row is 36 floats: the 16-byte read of lane l at row (l & 31), float 8 j + 4 (l >> 5) is conflict-free (16 rows x 36 words
 *      cover 64 banks once) and gives the lane its next four k-steps.  The k-step <-> column map is the same permutation on both
 *      operands, which a screen may use: any order is inside the margin.  Query blocks of one doc block are adjacent in the grid:
 *      the doc tile comes from HBM once and from L2 after that.  Epilogue: 16 compares per accumulator against the bounds held in
 *      LDS, one ballot; a kept pair fetches its filter bit, takes a slot of the query's buffer by a vector atomic add and writes
 *      the doc id.  A slot at or beyond SRX_F32_BATCHED_CAP sets the query's overflow flag.
 *   3. exact rescoring of the buffers (one wave per 64 candidates, the arithmetic above), + score_offset, > 0.
 *   4. rank: the buffers folded into exact top-k lists (topk_fold) and ranked (srx_merge_impl).
 *   5. fallback for overflowed queries only (all-tied or filter-starved rows): the exact arithmetic over the whole doc range,
 *      folded directly.  Slow, exact, and not launched into work unless some query overflowed.
 *
 * ---- constants ----------------------------------------------------------------------------------------------------------
 *
 * SRX_F32_BATCHED_CAP       entries of a query's candidate buffer (a doc id and, after rescoring, its ranked bits: 8 bytes).
 * SRX_F32_BATCHED_MIN_DOCS  below this many docs there is no sample (S = 0, tau = 0); MIN_DOCS <= CAP: no overflow there.
 * SRX_F32_BATCHED_TARGET    survivors per query the sample aims at.  A survivor costs a gathered row read (dim * 4 bytes), not
 *                           8 bytes as in the half index's fused search, so the aim is CAP / 8, not CAP / 3.
 * Sample rule: S = 0 if n_docs < MIN_DOCS; else
 *     S = min(max(ceil(k n_docs / TARGET), clamp(164 k, 4096, 16384)), 262144) rounded up to a multiple of 128; S = 0 if 4 S > n_docs.
 *
 * Workspace, each term rounded up to 256 bytes, plus 256, with qb = min(nq, 1024):
 *     norm, margins, bounds   256;  qb * 8;  qb * 4
 *     sample matrix           qb * S * 4
 *     lists                   3 terms: qb * L * k * 4 (docs), the same (scores), qb * L * 4 (counts), L = fallback splits =
 *                             clamp(ceil(n_docs / 256) / 16, 1, min(4096 / k, 64))
 *     counters                (qb * 32 + qb + 1) * 4 (a 128-byte line per buffer counter, the overflow flags, any-overflow)
 *     buffers                 2 terms of qb * CAP * 4 (docs, ranked bits)
 *
 * Not covered: a second threshold round; a cached row norm; a sharded dense corpus; the uint8 / INT8 indexes.
 */
#ifndef SPARSE_RX_F32_BATCHED_H
#define SPARSE_RX_F32_BATCHED_H

#include "sparse_rx_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRX_F32_BATCHED_CAP 65536
#define SRX_F32_BATCHED_MIN_DOCS 65536
#define SRX_F32_BATCHED_PASS 1024
#define SRX_F32_BATCHED_TARGET 8192
#define SRX_F32_BATCHED_MAX_SAMPLE 262144
#define SRX_F32_BATCHED_C 2.0
#define SRX_F32_BATCHED_MEASURED_RATIO 0.079657

int64_t srx_dense_f32_batched_workspace_bytes(int32_t nq, int64_t n_docs, int32_t k);

int srx_dense_search_f32_batched(int32_t device, const float *emb, int64_t n_docs, int32_t dim, const float *queries, int32_t nq,
                                 int32_t k, int64_t doc_base, const srx_doc_filter *filter /* NULL: none */, int32_t *out_doc,
                                 float *out_score, int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream,
                                 float score_offset);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_F32_BATCHED_H */
