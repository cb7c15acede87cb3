/* sparse_rx_half.h -- half-precision dense index: f16 / bf16 rows searched by MFMA, a whole query batch per GEMM.
 *
 * Fifth header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: the f32 search of sparse_rx.h streams the whole matrix once per pass of four queries, the INT8 search is fast but
 * lossy and takes no filter.  Half-precision rows are what most embedding stacks keep; they are half the bytes of f32, and
 * gfx950 multiplies them at the MFMA rate, so one GEMM serves a whole query batch -- with a filter, a score offset and a
 * scorer of given docs, as the f32 index has them.  The reference has no half-precision index: like the fusion, the scorers
 * of given docs and the filters, nothing here replaces reference code.
 *
 * ---- storage ----------------------------------------------------------------------------------------------------------
 *
 * The corpus lives ONLY in MFMA-fragment order, one layout for both types (16-bit elements): rows in tiles of 32, one
 * 16-byte piece per lane and k-step of v_mfma_f32_32x32x16_{f16,bf16}.  Lane l of k-step s of tile t holds row
 * 32 t + (l & 31), columns 16 s + 8 (l >> 5) .. + 7 -- the layout srx_dense_pack_i8 uses, at 16 columns per step.  With
 * KS = dim_pad / 16, element (row r, column c) is at BYTE offset
 *
 *     ((((r >> 5) * KS + (c >> 4)) * 64 + (r & 31) + 32 * ((c >> 3) & 1)) * 8 + (c & 7)) * 2.
 *
 * Rows past n_docs in the last tile are zeros, columns dim .. dim_pad - 1 are zeros.  dim_pad is a multiple of 64, at most
 * 1024 (as the f32 and uint8 calls).  srx_dense_half_bytes(n_rows, dim_pad) = ceil(n_rows / 32) * 32 * dim_pad * 2 is the
 * buffer size; SRX_ERR_INVALID for n_rows < 0 or a bad dim_pad.  The buffer is 16-byte aligned.
 *
 * ---- conversion -------------------------------------------------------------------------------------------------------
 *
 * srx_dense_convert_half converts a CHUNK of f32 rows, with the calling convention of srx_dense_quantize_i8 with
 * packed = 1 (sparse_rx_quant.h): emb holds rows row0 .. row0 + n_rows - 1 (row stride ld >= dim ELEMENTS, 4-byte alignment is
 * enough) of a corpus of n_total rows, out_packed is the buffer of the WHOLE corpus.  row0 % 32 == 0; a call writes every
 * byte of the 32-row tiles it covers (zeros for the rows of its last tile it does not hold), so only the chunk that ends
 * the corpus may end inside a tile.  No scales, no workspace; asynchronous on `stream`.
 *
 * Each value is rounded to the target type with round-to-nearest-even, half subnormals included: f16 output is bit-equal
 * to NumPy's astype(np.float16), bf16 output to torch's CPU .to(torch.bfloat16).  A row that holds a non-finite value, or a
 * value whose rounding is not finite (|x| >= 65520 for f16), is written as zeros and bit 0 (the value of
 * SRX_QUANT_NONFINITE) is ORed into *flag (i32[1] zeroed by the caller, or NULL; one vector atomic per wave that saw such
 * a row, nothing is written otherwise).
 *
 * ---- scores -----------------------------------------------------------------------------------------------------------
 *
 * Queries arrive as f32 [nq][dim_pad] (columns dim .. dim_pad - 1 zero), 16-byte aligned; the search rounds them to the
 * corpus type with the same rounding.  score[q][d] is the fp32 accumulator of ONE chain of the MFMA instruction
 * v_mfma_f32_32x32x16_{f16,bf16} over the k-steps s = 0, 1, ..., dim_pad / 16 - 1 in ascending order, starting from
 * +0.0f: no split-K, no partial sums combined afterwards.  The order and the rounding INSIDE one instruction are the
 * hardware's; they are not restated here or anywhere in this project.  What follows from the above:
 *   - scores are deterministic;
 *   - the score bits of a (query, doc) pair do not depend on nq, on the other queries, on the doc's row number, on k, on
 *     a filter, or on which of the two entry points below computed them.  (This rests on the hardware computing each output
 *     element from its own row and column operands only; the tests check it.)
 *   - the result is exact whenever every product and partial sum is representable in fp32 (small integers, for one).
 * Not specified: half-subnormal inputs and non-finite queries are as the instruction treats them.
 *
 * ---- srx_dense_search_half ---------------------------------------------------------------------------------------------
 *
 * The rules of sparse_rx.h's srx_dense_search_f32: the ranked value is fl32(score + score_offset); only values > 0 are
 * results; order (value descending, doc ascending); ids doc_base + row; rows padded with -1 / +0.0f; every word of every
 * row and every count is written; 1 <= k <= SRX_MAX_K.  A non-NULL `filter` has the semantics of sparse_rx_filter.h: its
 * rows are over the n_docs rows of the corpus, q_filter NULL / -1 / row.  The workspace is
 * srx_dense_half_workspace_bytes(nq, n_docs, k): the packed query block and the fp32 score matrix of one pass of up to
 * 1024 queries, and the candidate lists of the row splits.  A pass holds as many queries as keep the matrix within 4 GiB, but
 * never fewer than 32: the matrix is min(nq, 1024) rows while n_docs <= 2^20, at most 4 GiB while n_docs <= 2^25, and
 * 32 rows = 128 bytes per doc beyond that (256 GiB at 2^31 docs; the workspace call returns the size, the caller decides).
 *
 * ---- srx_dense_score_docs_half ----------------------------------------------------------------------------------------
 *
 * The contract of sparse_rx_rescore.h's srx_dense_score_docs_f32: cand_doc i32[nq][m] GLOBAL ids, cand_count i32[nq] or
 * NULL, out_score f32[nq][m] with every word written; padding (-1, entries at or beyond cand_count[q]) and ids outside
 * [doc_base, doc_base + n_docs) give +0.0f; no > 0 filter, no offset; duplicates are legal; m is limited only by
 * nq * m <= 2^31 - 1.  The candidate rows are gathered from the packed corpus and go through the same instruction chain,
 * so the scores are bit-equal to those the search returns (at score_offset 0).  No workspace.
 *
 * ---- refusals ---------------------------------------------------------------------------------------------------------
 *
 * SRX_ERR_INVALID before anything touches a device: a type outside srx_half_type; dim_pad not a multiple of 64 in
 * [64, 1024]; convert: negative n_rows / row0 / n_total, row0 + n_rows > n_total, dim outside [1, dim_pad], ld < dim,
 * row0 % 32 != 0, more than 2^31 - 1 tiles in one call, and with n_rows > 0 a NULL emb / out_packed, an emb that is not
 * 4-byte aligned, an out_packed that is not 16-byte aligned; search: nq < 0, n_docs <= 0, k outside 1 .. 1024, a negative
 * doc_base or doc_base + n_docs >= 2^31 - 1, with nq > 0 a NULL pointer or a corpus / query block that is not 16-byte
 * aligned, and the filter rules of sparse_rx_filter.h (NULL bits, misaligned bits, n_filters < 1); score_docs: nq < 0,
 * m < 1, nq * m > 2^31 - 1, n_docs outside [1, 2^31 - 2], a negative doc_base, with nq > 0 a NULL or misaligned pointer
 * as above.  SRX_ERR_NOMEM: a NULL or too small workspace.  nq == 0 and n_rows == 0 return SRX_OK without a launch.
 */
#ifndef SPARSE_RX_HALF_H
#define SPARSE_RX_HALF_H

#include "sparse_rx.h"
#include "sparse_rx_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { SRX_HALF_F16 = 0, SRX_HALF_BF16 = 1 } srx_half_type;

int64_t srx_dense_half_bytes(int64_t n_rows, int32_t dim_pad);

int srx_dense_convert_half(int32_t device, int32_t type, const float *emb, int64_t ld, int64_t n_rows, int32_t dim, int32_t dim_pad,
                           int64_t row0, int64_t n_total, void *out_packed, int32_t *flag, void *stream);

int64_t srx_dense_half_workspace_bytes(int32_t nq, int64_t n_docs, int32_t k);

int srx_dense_search_half(int32_t device, int32_t type, const void *corpus_packed, int64_t n_docs, int32_t dim_pad,
                          const float *queries, int32_t nq, int32_t k, int64_t doc_base, const srx_doc_filter *filter /* NULL: none */,
                          int32_t *out_doc, float *out_score, int32_t *out_count, void *workspace, int64_t workspace_bytes,
                          void *stream, float score_offset);

int srx_dense_score_docs_half(int32_t device, int32_t type, const void *corpus_packed, int64_t n_docs, int32_t dim_pad,
                              const float *queries, int32_t nq, int64_t doc_base, const int32_t *cand_doc, const int32_t *cand_count,
                              int32_t m, float *out_score, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_HALF_H */
