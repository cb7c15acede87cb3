/* sparse_rx_pq.h -- PQ dense index: 8-bit product codes, a per-query score table, a table-lookup scan, scores of given docs.
 *
 * Twentieth header of libsparse_rx.so (same library, same conventions as sparse_rx_half.h: extern "C", device pointers,
 * negative return codes, the message of the last failure from the error-text call of sparse_rx.h; every refusal happens
 * before anything touches a device; asynchronous on `stream`; nothing is allocated).
 *
 * Why: the other dense storages cost 3 072 (f32), 1 536 (f16), 792 / 408 (MX) or 96 (binary) bytes per 768-dim row, and only
 * the 96-byte one saves much memory -- at a Hamming distance's recall.  Product quantisation turns every dsub consecutive
 * dimensions into ONE byte, the index of the nearest of 256 codewords of that subspace; a query scores a row by adding
 * M = ceil(dim / dsub) entries of a table it computes once.  At dsub = 8 a 768-dim row is the same 96 bytes and the score
 * approximates the inner product.  The reference has no PQ index: nothing here replaces reference code.
 *
 * ---- geometry ---------------------------------------------------------------------------------------------------------
 *
 * dsub in {4, 8, 16}; 1 <= dim <= 1024; M = ceil(dim / dsub), 1 <= M <= 128; 256 codewords per subspace, always.
 * codebooks is f32[M][256][dsub], plain layout, 16-byte aligned.  It is DATA: the caller fixes it once (the Python layer
 * trains it with Lloyd's iteration) and passes the same array to every call.  Columns dim .. M * dsub - 1 are zeros in rows
 * and queries: the kernels supply them and never read a row or a query past dim.  The codebooks' entries at those columns
 * are used as given.
 *
 * ---- codes ------------------------------------------------------------------------------------------------------------
 *
 * M_pad = M rounded up to a multiple of 16.  tiled = 1 (the corpus): tiles of 64 rows, one 16-byte piece per lane.  Piece p
 * (codes 16 p .. 16 p + 15) of row r is at byte
 *
 *     (((r >> 6) * (M_pad / 16) + p) * 64 + (r & 63)) * 16 ;
 *
 * code 16 p + b is byte b of the piece.  Bytes M .. M_pad - 1 and the rows past n_total of the last tile are zeros and are
 * never looked up.  srx_pq_bytes(n_rows, M) = ceil(n_rows / 64) * 64 * M_pad is the buffer size (SRX_ERR_INVALID for
 * n_rows < 0 or M outside 1 .. 128); the buffer is 16-byte aligned.  Every offset is 64-bit.  tiled = 0: plain u8[n][M].
 *
 * ---- arithmetic (the contract) ----------------------------------------------------------------------------------------
 *
 * There is no tolerance.  Every operation below is ONE fp32 operation rounded on its own (no FMA), fl() is that rounding.
 *
 *   encode  for row x, subspace m and codeword c, d(c) is the sequential sum from +0.0f over j = 0 .. dsub - 1 ascending of
 *           fl(t * t) with t = fl(x[m dsub + j] - C[m][c][j]).  The code is found by: best = +inf, code = 0; for c = 0 .. 255
 *           ascending, if d(c) < best then best = d(c), code = c.  So ties go to the lowest code and a NaN distance never wins.
 *           Non-finite inputs give unspecified codes in [0, 255] and touch nothing out of bounds.
 *   table   LUT[q][m][c] is the sequential sum from +0.0f over j ascending of fl(q[m dsub + j] * C[m][c][j]).  Queries are f32
 *           and are not rounded to any other type.
 *   score   score[q][d] is the sequential sum from +0.0f over m = 0 .. M - 1 ascending of LUT[q][m][code[d][m]].
 *
 * So the bits of a (query, doc) score do not depend on nq, on the other queries, on k, on a filter, on the launch geometry
 * or on which entry point computed them.
 *
 * ---- srx_pq_encode ----------------------------------------------------------------------------------------------------
 *
 * Encodes a CHUNK of f32 rows with the calling convention of srx_binary_encode: x holds rows row0 .. row0 + n_rows - 1 (row
 * stride ld >= dim ELEMENTS, 4-byte alignment is enough) of a set of n_total rows, out_codes is the buffer of the WHOLE set.
 * With tiled = 1, row0 % 64 == 0 and a call writes every byte of the 64-row tiles it covers (zeros for the rows of its last
 * tile it does not hold and for bytes M .. M_pad - 1), so only the chunk that ends the corpus may end inside a tile.  With
 * tiled = 0 a call writes the M bytes of each of its rows and nothing else; row0 is free.
 *
 * ---- srx_pq_lut -------------------------------------------------------------------------------------------------------
 *
 * queries f32[nq] rows of stride ldq >= dim elements -> out_lut f32[nq][M][256], the table above.
 *
 * ---- srx_pq_search ----------------------------------------------------------------------------------------------------
 *
 * The rules of srx_dense_search_half.  codes is a corpus of n_docs rows (tiled = 1); queries f32 rows of stride ldq >= dim.
 * The ranked value of doc d is fl32(score[q][d] + score_offset); only values > 0 are results.  Row q of the outputs holds
 * the count[q] = min(k, results) best by (value descending, doc ascending): out_doc = doc_base + row, out_score = the
 * ranked value; the rest of the row is -1 / +0.0f; every word of every row and every count is written.  1 <= k <= SRX_MAX_K.
 * A non-NULL `filter` has the semantics of sparse_rx_filter.h: its rows are over the n_docs rows of the corpus, q_filter
 * NULL / -1 / row; a row that allows nothing gives count 0.
 *
 * The workspace is srx_pq_workspace_bytes(nq, n_docs, M, k).  With ld = ceil(n_docs / 64) * 64,
 * QB = clamp(floor(2^32 / (4 ld) / 32) * 32, 32, 1024) queries per pass, qb = min(nq, QB),
 * ns = max(1, min(2048 / max(qb, 1), n_docs / 16384, 4096 / k)) splits of a score row (integer divisions; the plan of the
 * half index) and r256(x) = x rounded up to a multiple of 256, it is
 *
 *     r256(1024 qb M) + r256(4 qb ld) + 2 r256(4 qb ns k) + r256(4 qb ns) + 256 :
 *
 * the tables of one pass, its fp32 score matrix and the candidate lists (docs, values, counts) of the row splits.
 *
 * ---- srx_pq_score_docs ------------------------------------------------------------------------------------------------
 *
 * The candidate contract of srx_dense_score_docs_half: cand_doc i32[nq][m] GLOBAL ids, cand_count i32[nq] or NULL,
 * out_score f32[nq][m] with every word written; padding (-1, entries at or beyond cand_count[q]) and ids outside
 * [doc_base, doc_base + n_docs) give +0.0f; duplicates are legal; m is limited only by nq * m <= 2^31 - 1.  No offset and
 * no > 0 rule: the bits are those of the search at score_offset 0.  No workspace.
 *
 * ---- refusals ---------------------------------------------------------------------------------------------------------
 *
 * SRX_ERR_INVALID before anything touches a device: dsub outside {4, 8, 16}; dim outside 1 .. 1024; M > 128;
 * encode: tiled outside {0, 1}, negative n_rows / row0 / n_total, row0 + n_rows > n_total, ld < dim, row0 % 64 != 0 with
 * tiled = 1, more than 2^31 - 1 tiles in one call, and with n_rows > 0 a NULL x / codebooks / out_codes, an x that is not
 * 4-byte aligned, codebooks that are not 16-byte aligned, an out_codes that is not 16-byte aligned with tiled = 1;
 * lut: nq < 0, ldq < dim, and with nq > 0 a NULL pointer, queries that are not 4-byte aligned, codebooks / out_lut that are
 * not 16-byte aligned; search: nq < 0, n_docs <= 0, k outside 1 .. 1024, ldq < dim, a negative doc_base or
 * doc_base + n_docs >= 2^31 - 1, with nq > 0 a NULL pointer, codes / codebooks that are not 16-byte aligned, queries that
 * are not 4-byte aligned, and the filter rules of sparse_rx_filter.h (NULL bits, misaligned bits, n_filters < 1);
 * score_docs: nq < 0, m < 1, nq * m > 2^31 - 1, n_docs outside [1, 2^31 - 2], ldq < dim, a negative doc_base, with nq > 0 a
 * NULL or misaligned pointer as above; workspace_bytes: nq < 0, n_docs <= 0, M outside 1 .. 128, k outside 1 .. 1024.
 * SRX_ERR_NOMEM: a NULL or too small workspace.  nq == 0 and n_rows == 0 return SRX_OK without a launch.
 *
 * There is no device call for the training: Lloyd's iteration is srx_pq_encode (tiled = 0) plus the centroid update of
 * sparse_rx_ivf.h on each subspace's columns, driven by the caller.
 */
#ifndef SPARSE_RX_PQ_H
#define SPARSE_RX_PQ_H

#include "sparse_rx.h"
#include "sparse_rx_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t srx_pq_bytes(int64_t n_rows, int32_t M);

int srx_pq_encode(int32_t device, const float *x, int64_t ld, int64_t n_rows, int32_t dim, int32_t dsub, int64_t row0, int64_t n_total,
                  const float *codebooks, int32_t tiled, void *out_codes, void *stream);

int srx_pq_lut(int32_t device, const float *codebooks, int32_t dim, int32_t dsub, const float *queries, int64_t ldq, int32_t nq,
               float *out_lut, void *stream);

int64_t srx_pq_workspace_bytes(int32_t nq, int64_t n_docs, int32_t M, int32_t k);

int srx_pq_search(int32_t device, const void *codes, int64_t n_docs, int32_t dim, int32_t dsub, const float *codebooks,
                  const float *queries, int64_t ldq, int32_t nq, int32_t k, int64_t doc_base, const srx_doc_filter *filter /* NULL: none */,
                  int32_t *out_doc, float *out_score, int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream,
                  float score_offset);

int srx_pq_score_docs(int32_t device, const void *codes, int64_t n_docs, int32_t dim, int32_t dsub, const float *codebooks,
                      const float *queries, int64_t ldq, int32_t nq, int64_t doc_base, const int32_t *cand_doc, const int32_t *cand_count,
                      int32_t m, float *out_score, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_PQ_H */
