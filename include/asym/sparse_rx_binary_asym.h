/* sparse_rx_binary_asym.h -- binary dense index, asymmetric scores: the docs stay at one bit per dimension, the query keeps
 * four (a sign and three bits of magnitude), and the corpus is ranked by the integer inner product of the two.
 *
 * Twenty-fifth header of libsparse_rx.so (same library, same conventions as binary/sparse_rx_binary.h: extern "C", device
 * pointers, negative return codes, the message of the last failure from the error-text call of sparse_rx.h; every refusal
 * happens before anything touches a device; asynchronous on `stream`; nothing is allocated).
 *
 * Why: the Hamming search of sparse_rx_binary.h keeps only the signs of the query.  Here the corpus is THE SAME tiled 1-bit
 * buffer srx_binary_encode writes (unchanged, not copied: no extra resident byte), and only the query is finer.  The score
 * estimates the inner product, the project's metric.  Everything below is integer work: the contract has no tolerance.  The
 * reference has no binary index: nothing here replaces reference code.  dim_pad and W = dim_pad / 32 are as in
 * sparse_rx_binary.h.
 *
 * ---- srx_binary_asym_quantize ---------------------------------------------------------------------------------------------
 *
 * q f32[nq][ld] (row stride ld >= dim ELEMENTS, 4-byte alignment is enough), center f32[dim] or NULL (zeros), out_codes
 * i8[nq][dim_pad], 16-byte aligned.  Every step is ONE fp32 operation (round to nearest even, subnormals kept):
 *
 *     r[c]    = fl(q[c] - center[c])                     c < dim
 *     amax    = the largest |r[c]| that is not NaN, or 0 if there is none
 *     inv     = amax > 0 ? fl(7 / amax) : 0
 *     code[c] = clamp(rint(fl(r[c] * inv)), -7, 7)       rint to nearest even; a NaN product gives 0
 *     code[c] = 0                                        dim <= c < dim_pad
 *
 * So an amax of 0 or +inf gives all-zero codes (inv = 0; inf * 0 is NaN), and a subnormal amax gives inv = +inf and codes in
 * {-7, 0, 7}.  The scale amax / 7 is NOT an output: it is one positive factor per query and cannot change that query's ranking.
 *
 * ---- score ----------------------------------------------------------------------------------------------------------------
 *
 *     s(q, d) = sum over c < dim_pad of code_q[c] * (2 b_d[c] - 1),       an int32 in [-7 dim_pad, 7 dim_pad].
 *
 * ---- srx_binary_asym_search -----------------------------------------------------------------------------------------------
 *
 * The argument list and output contract of srx_binary_search with q_codes i8[nq][dim_pad] for q_bits and out_score for
 * out_dist: for each query the m allowed docs best by (score descending, doc ascending); out_doc i32[nq][m] = doc_base + row,
 * out_score i32[nq][m], out_count i32[nq] = min(m, allowed docs).  Every allowed doc is rankable (there is no > 0 rule).  Rows
 * are padded with doc -1 / score INT32_MIN; every word of every row and every count is written.  1 <= m <= SRX_MAX_K.  The
 * filter and q_filter follow sparse_rx_filter.h, doc_base behaves as in srx_binary_search.  q_codes are READ as codes: a byte
 * outside [-7, 7] is not refused and not defined.
 *
 * route: 0 = the library chooses by nq (the bit-plane route below SRX_BINARY_ASYM_ROUTE_NQ = 16 queries, the MFMA route from
 * there), 1 = the bit-plane route, 2 = the MFMA route.  Both routes compute the same integers and rank them with the same
 * kernels: they return identical words for every input.
 *
 * The workspace is srx_binary_asym_workspace_bytes(nq, n_docs, m, dim_pad).  With ld, QB, qb, ns and r256 as in
 * sparse_rx_binary.h (ld = ceil(n_docs / 64) * 64, QB = clamp(floor(2^32 / (2 ld) / 32) * 32, 32, 1024), qb = min(nq, QB),
 * ns = max(1, min(2048 / max(qb, 1), n_docs / 16384, 4096 / m))) and q32 = qb rounded up to a multiple of 32 it is
 *
 *     r256(2 qb ld) + 2 r256(4 qb ns m) + r256(4 qb ns) + r256(4 qb m) + r256(q32 dim_pad) + r256(4 q32) + 256 :
 *
 * the pass plan of srx_binary_search (the u16 matrix of one pass, the split lists, the ranked values) plus the pass's
 * prepared queries -- q32 dim_pad bytes hold either the four plane words per 32 dimensions (qb dim_pad / 2 bytes) or the codes
 * in MFMA operand order -- and their code sums.
 *
 * ---- srx_binary_asym_score_docs -------------------------------------------------------------------------------------------
 *
 * The candidate contract of srx_binary_dist_docs: cand_doc i32[nq][m] GLOBAL ids, cand_count i32[nq] or NULL, out_score
 * i32[nq][m] with every word written; padding (-1, entries at or beyond cand_count[q]) and ids outside
 * [doc_base, doc_base + n_docs) give INT32_MIN; duplicates are legal; m is limited only by nq * m <= 2^31 - 1.  The scores are
 * those the search returns.  No workspace.
 *
 * ---- refusals -------------------------------------------------------------------------------------------------------------
 *
 * SRX_ERR_INVALID before anything touches a device: dim_pad not a multiple of 128 in [128, 1024]; quantize: nq < 0, dim
 * outside [1, dim_pad], ld < dim, and with nq > 0 a NULL q / out_codes, a q or center that is not 4-byte aligned, an out_codes
 * that is not 16-byte aligned; search: a route outside {0, 1, 2}, nq < 0, n_docs <= 0, m outside 1 .. 1024, a negative
 * doc_base or doc_base + n_docs >= 2^31 - 1, with nq > 0 a NULL pointer or a corpus / q_codes that is not 16-byte aligned, and
 * the filter rules of sparse_rx_filter.h; score_docs: nq < 0, m < 1, nq * m > 2^31 - 1, n_docs outside [1, 2^31 - 2], a
 * negative doc_base, with nq > 0 a NULL or misaligned pointer as above; workspace_bytes: nq < 0, n_docs <= 0, m outside
 * 1 .. 1024, a bad dim_pad.  SRX_ERR_NOMEM: a NULL or too small workspace.  nq == 0 returns SRX_OK without a launch.
 */
#ifndef SPARSE_RX_BINARY_ASYM_H
#define SPARSE_RX_BINARY_ASYM_H

#include "sparse_rx.h"
#include "sparse_rx_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRX_BINARY_ASYM_ROUTE_NQ 16 /* route 0: the MFMA route from this many queries */

int srx_binary_asym_quantize(int32_t device, const float *q, int64_t ld, int32_t nq, int32_t dim, int32_t dim_pad,
                             const float *center /* NULL: zeros */, int8_t *out_codes, void *stream);

int64_t srx_binary_asym_workspace_bytes(int32_t nq, int64_t n_docs, int32_t m, int32_t dim_pad);

int srx_binary_asym_search(int32_t device, const void *bits_tiled, int64_t n_docs, int32_t dim_pad, const int8_t *q_codes, int32_t nq,
                           int32_t m, int64_t doc_base, const srx_doc_filter *filter /* NULL: none */, int32_t *out_doc,
                           int32_t *out_score, int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream, int32_t route);

int srx_binary_asym_score_docs(int32_t device, const void *bits_tiled, int64_t n_docs, int32_t dim_pad, const int8_t *q_codes, int32_t nq,
                               int64_t doc_base, const int32_t *cand_doc, const int32_t *cand_count, int32_t m, int32_t *out_score,
                               void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_BINARY_ASYM_H */
