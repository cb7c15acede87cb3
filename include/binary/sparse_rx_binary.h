/* sparse_rx_binary.h -- binary dense index: one bit per dimension, Hamming top-m, distances of given docs.
 *
 * Seventeenth header of libsparse_rx.so (same library, same conventions as sparse_rx_half.h: extern "C", device pointers,
 * negative return codes, the message of the last failure from the error-text call of sparse_rx.h; every refusal happens
 * before anything touches a device; asynchronous on `stream`; nothing is allocated).
 *
 * Why: every other dense storage reads at least one byte per dimension per doc on every search.  One bit per dimension is
 * 32 times fewer bytes than f32 and 8 times fewer than INT8; the Hamming distance of the codes screens the corpus, and the
 * short pool it leaves is rescored from the exact rows (the Python layer does that with the scorers of given docs this
 * library already has).  The screen is integer work: its contract below has no tolerance.  The reference has no binary
 * index: nothing here replaces reference code.
 *
 * ---- codes ------------------------------------------------------------------------------------------------------------
 *
 * Bit c of a row is 1 iff x[c] > center[c], an fp32 compare; center == NULL means 0 for every column.  So NaN, -0.0 and
 * x == center give 0 and +inf gives 1 (unless the centre is +inf or NaN); there is no flag.  dim_pad = dim rounded up to a
 * multiple of 128, 128 <= dim_pad <= 1024, W = dim_pad / 32 words per row.  Column c is bit c & 31 of word c >> 5; the bits
 * at or above dim are 0, in docs and queries alike.  The centre is DATA: the caller fixes it once (the column means, for
 * one) and passes the same array for docs and queries.
 *
 * ---- layouts ----------------------------------------------------------------------------------------------------------
 *
 * tiled = 1 (the corpus): tiles of 64 rows, one 16-byte piece per lane and step of 128 columns.  Word w of row r is the
 * u32 at index
 *
 *     (((r >> 6) * (W / 4) + (w >> 2)) * 64 + (r & 63)) * 4 + (w & 3).
 *
 * Rows past n_total in the last tile are zeros.  tiled = 0 (queries): plain u32[n][W].
 * srx_binary_bytes(n_rows, dim_pad, tiled) = (tiled ? ceil(n_rows / 64) * 64 : n_rows) * W * 4 is the buffer size;
 * SRX_ERR_INVALID for n_rows < 0, a bad dim_pad or a tiled outside {0, 1}.  The buffers are 16-byte aligned.
 *
 * ---- srx_binary_encode ------------------------------------------------------------------------------------------------
 *
 * Encodes a CHUNK of f32 rows, with the calling convention of srx_dense_convert_half: x holds rows row0 .. row0 + n_rows - 1
 * (row stride ld >= dim ELEMENTS, 4-byte alignment is enough) of a set of n_total rows, out_bits is the buffer of the WHOLE
 * set.  center is f32[dim] or NULL.  With tiled = 1, row0 % 64 == 0 and a call writes every word of the 64-row tiles it
 * covers (zeros for the rows of its last tile it does not hold), so only the chunk that ends the corpus may end inside a
 * tile.  With tiled = 0 a call writes the W words of each of its rows and nothing else; row0 is free.
 *
 * ---- srx_binary_search ------------------------------------------------------------------------------------------------
 *
 * bits_tiled is a corpus of n_docs rows (tiled = 1), q_bits u32[nq][W] (tiled = 0).  dist(q, d) = popcount(q XOR d) over
 * the W words, in [0, dim_pad].  For each query the m allowed docs nearest by (distance ascending, doc ascending):
 * out_doc i32[nq][m] = doc_base + row, out_dist i32[nq][m], out_count i32[nq] = min(m, allowed docs).  Every doc is
 * rankable: there is no > 0 rule.  Rows are padded with doc -1 / distance -1; every word of every row and every count is
 * written.  1 <= m <= SRX_MAX_K.  A non-NULL `filter` has the semantics of sparse_rx_filter.h: its rows are over the n_docs
 * rows of the corpus, q_filter NULL / -1 / row; a row that allows nothing gives count 0.
 *
 * The workspace is srx_binary_workspace_bytes(nq, n_docs, m).  With ld = ceil(n_docs / 64) * 64,
 * QB = clamp(floor(2^32 / (2 ld) / 32) * 32, 32, 1024) queries per pass, qb = min(nq, QB),
 * ns = max(1, min(2048 / max(qb, 1), n_docs / 16384, 4096 / m)) splits of a distance row (integer divisions), and
 * r256(x) = x rounded up to a multiple of 256, it is
 *
 *     r256(2 qb ld) + 2 r256(4 qb ns m) + r256(4 qb ns) + r256(4 qb m) + 256 :
 *
 * the u16 distance matrix of one pass, the candidate lists (docs, values, counts) of the row splits, and the ranked values
 * of the pass before they are turned back into distances.
 *
 * ---- srx_binary_dist_docs ---------------------------------------------------------------------------------------------
 *
 * The candidate contract of srx_dense_score_docs_half: cand_doc i32[nq][m] GLOBAL ids, cand_count i32[nq] or NULL,
 * out_dist i32[nq][m] with every word written; padding (-1, entries at or beyond cand_count[q]) and ids outside
 * [doc_base, doc_base + n_docs) give -1; duplicates are legal; m is limited only by nq * m <= 2^31 - 1.  The distances
 * are those the search returns.  No workspace.
 *
 * ---- refusals ---------------------------------------------------------------------------------------------------------
 *
 * SRX_ERR_INVALID before anything touches a device: dim_pad not a multiple of 128 in [128, 1024]; tiled outside {0, 1};
 * encode: negative n_rows / row0 / n_total, row0 + n_rows > n_total, dim outside [1, dim_pad],
 * ld < dim, row0 % 64 != 0 with tiled = 1, more than 2^31 - 1 tiles in one call, and with n_rows > 0 a NULL x / out_bits, an
 * x or center that is not 4-byte aligned, an out_bits that is not 16-byte aligned; search: nq < 0, n_docs <= 0, m outside
 * 1 .. 1024, a negative doc_base or doc_base + n_docs >= 2^31 - 1, with nq > 0 a NULL pointer or a corpus / query block
 * that is not 16-byte aligned, and the filter rules of sparse_rx_filter.h (NULL bits, misaligned bits, n_filters < 1);
 * dist_docs: nq < 0, m < 1, nq * m > 2^31 - 1, n_docs outside [1, 2^31 - 2], a negative doc_base, with nq > 0 a NULL or
 * misaligned pointer as above; workspace_bytes: nq < 0, n_docs <= 0, m outside 1 .. 1024.  SRX_ERR_NOMEM: a NULL or too
 * small workspace.  nq == 0 and n_rows == 0 return SRX_OK without a launch.
 *
 * There is no device call for the centre: the column means are taken by the caller (the Python layer uses torch) and are
 * input data from then on.
 */
#ifndef SPARSE_RX_BINARY_H
#define SPARSE_RX_BINARY_H

#include "sparse_rx.h"
#include "sparse_rx_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t srx_binary_bytes(int64_t n_rows, int32_t dim_pad, int32_t tiled);

int srx_binary_encode(int32_t device, const float *x, int64_t ld, int64_t n_rows, int32_t dim, int32_t dim_pad, int64_t row0,
                      int64_t n_total, const float *center /* NULL: zeros */, int32_t tiled, void *out_bits, void *stream);

int64_t srx_binary_workspace_bytes(int32_t nq, int64_t n_docs, int32_t m);

int srx_binary_search(int32_t device, const void *bits_tiled, int64_t n_docs, int32_t dim_pad, const uint32_t *q_bits, int32_t nq,
                      int32_t m, int64_t doc_base, const srx_doc_filter *filter /* NULL: none */, int32_t *out_doc, int32_t *out_dist,
                      int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream);

int srx_binary_dist_docs(int32_t device, const void *bits_tiled, int64_t n_docs, int32_t dim_pad, const uint32_t *q_bits, int32_t nq,
                         int64_t doc_base, const int32_t *cand_doc, const int32_t *cand_count, int32_t m, int32_t *out_dist,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_BINARY_H */
