/* sparse_rx_mx.h -- MX dense index: OCP microscaling rows (MXFP8 e4m3 / MXFP4 e2m1, one e8m0 scale per 32 columns) searched
 * by the block-scaled MFMA of gfx950, v_mfma_scale_f32_32x32x64_f8f6f4.
 *
 * Eighteenth header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).  The reference has no such index:
 * nothing here replaces reference code.
 *
 * Why: between f16 (2 bytes per dim) and the binary codes (1 bit) there was no storage that is accurate AND accepted at every
 * door the half index serves.  An MXFP8 row of 768 dims is 792 bytes, an MXFP4 row 408 (f16: 1536); a block of 32 columns
 * keeps its own dynamic range.  The entry points take a filter, a score offset and given docs as srx_dense_*_half do.
 *
 * ---- formats (srx_mx_type) ----------------------------------------------------------------------------------------------
 *
 * SRX_MX_FP8: elements OCP e4m3 (bias 7, 3 mantissa bits, subnormals, finite maximum 448 = code 0x7E, emax 8; the NaN code
 * 0x7F is never written).  SRX_MX_FP4: elements e2m1 (values 0, .5, 1, 1.5, 2, 3, 4, 6 = codes 0 .. 7, bit 3 the sign;
 * emax 2).  One e8m0 scale code per 32 consecutive columns of a row: the block's value is element * 2^(code - 127).
 *
 * The quantiser, pinned bit for bit (tests/mx_ref.py restates it).  For each block of 32 columns, amax its largest |x|:
 *   e = clamp(expfield(amax) - 127 - emax, -127, 127), code = e + 127, where expfield is bits 30 .. 23 of the f32 (0 for an
 *   f32 subnormal); an all-zero block has code 127.  Every element is v = x * 2^(-e): exact, a power-of-two scaling (computed
 *   in fp32; a product below 2^-126 is inexact there, but it is then below half the smallest element of either format and
 *   rounds to zero as the exact value does).  v is clamped to +-max, then rounded to the nearest element value, ties to the
 *   even code; a value that rounds to zero is stored as code 0 (no negative zero).
 * A row that holds a NaN or an inf is written as zeros with every scale 127 and SRX_QUANT_NONFINITE (sparse_rx_quant.h) is
 * ORed into *flag, as srx_dense_convert_half does; every finite f32 row is representable, nothing else is refused.
 *
 * Queries are ALWAYS quantised to MXFP8 by the same rule, for both corpus types (the instruction multiplies FP8 x FP4).  A
 * query row that holds a NaN or an inf becomes zeros.
 *
 * ---- storage: fragment order only, one buffer -----------------------------------------------------------------------------
 *
 * dim_pad is a multiple of 64 in [64, 1024], KS = dim_pad / 64 k-steps, rows in tiles of 32, T = ceil(n_rows / 32) tiles.
 * The codes come first, the scales follow at byte T * 32 * dim_pad * bits / 8 (bits = 8 or 4).
 *   codes   piece (tile t, k-step s, lane l) holds codes of row 32 t + (l & 31), at byte ((t * KS + s) * 64 + l) * P; h = l >> 5.
 *           FP8, P = 32, one byte per column: bytes 0 .. 15 are columns 64 s + 16 h .. + 15 (of the k-step's first block),
 *           bytes 16 .. 31 columns 64 s + 32 + 16 h .. + 15 (of its second block): a lane holds 16 columns of EACH block.
 *           FP4, P = 16: columns 64 s + 32 h .. + 31 ascending, column 2 i of them the low nibble of byte i, 2 i + 1 the high.
 *   scales  SG = ceil(KS / 4) dwords per lane and tile: byte ((t * SG + (s >> 2)) * 64 + l) * 4 + (s & 3) is the scale code of
 *           columns 64 s + 32 (l >> 5) .. + 31 of row 32 t + (l & 31) -- the lane owns the scale of block l >> 5 of the
 *           k-step, for FP8 too; bytes of k-steps >= KS are 127.
 * Rows past n_rows and columns past dim are zero codes (their blocks' scales 127).
 * srx_mx_bytes(type, n_rows, dim_pad) = T * 32 * dim_pad * bits / 8 + T * SG * 256.  The buffer is 16-byte aligned.
 * This is the operand order of the instruction as measured on an MI355X with one-hot and stepped rows (it is not the order
 * first assumed from the instruction's description, 32 ascending columns per lane for FP8: that gave wrong scores at every
 * shape): a lane's piece is its 8 (FP8) or 4 (FP4) operand registers, byte 0 first; an FP8 operand's registers 0 .. 3 are
 * scaled by the scale of lane (l & 31) and registers 4 .. 7 by that of lane (l & 31) + 32, an FP4 operand's four registers by
 * the lane's own; the scale register is the dword, the byte picked by op_sel = s & 3.  Nothing is repacked at search time.
 *
 * ---- srx_mx_convert -------------------------------------------------------------------------------------------------------
 *
 * The calling convention of srx_dense_convert_half: emb holds rows row0 .. row0 + n_rows - 1 (row stride ld >= dim ELEMENTS,
 * 4-byte aligned) of a corpus of n_total rows, out is the buffer of the WHOLE corpus (the scales' place depends on n_total).
 * row0 % 32 == 0; a call writes every byte, codes and scales, of the 32-row tiles it covers, so only the chunk that ends the
 * corpus may end inside a tile.  No workspace; asynchronous on `stream`.
 *
 * ---- scores ---------------------------------------------------------------------------------------------------------------
 *
 * Queries arrive as f32 [nq][dim_pad] (columns dim .. dim_pad - 1 zero), 16-byte aligned.  score[q][d] is the fp32 accumulator
 * of ONE chain of the scaled MFMA over the k-steps s = 0, 1, ..., KS - 1 ascending, from +0.0f, each k-step fed its own two
 * scale bytes: no split-K.  The order and rounding inside one instruction are the hardware's.  As in sparse_rx_half.h: scores
 * are deterministic; the score bits of a (query, doc) pair do not depend on nq, on the other queries, on the doc's row
 * number, on k, on a filter, or on which entry point computed them.  Observed on an MI355X: scores of small integers (FP8
 * rows and queries in [-15, 15], FP4 rows in +-{0 .. 6}, differing scales along a row, dim_pad 64 .. 1024) equal the integer dot
 * products bit for bit; on Gaussian rows with a per-block spread of 2^+-6 the error against the exact dot product of the
 * dequantised operands is about 2^-17 of sum |q_i d_i| at dim_pad 256 (within dim_pad * 2^-22 * sum |q_i d_i|), which is MORE than an
 * fp32 chain loses: the instruction does not add its 64 products with fp32 precision, and rows that mix blocks of very different
 * magnitude exceeded that bound up to 3.2 times.
 *
 * srx_mx_search: the argument list and rules of srx_dense_search_half: ranked value fl32(score + score_offset), > 0 only,
 * (value descending, doc ascending), ids doc_base + row, rows padded with -1 / +0.0f, optional srx_doc_filter,
 * 1 <= k <= SRX_MAX_K, passes of up to 1024 queries.  srx_mx_workspace_bytes(nq, n_docs, k) equals
 * srx_dense_half_workspace_bytes(nq, n_docs, k): the packed query block, the fp32 score matrix of one pass, the row splits'
 * candidate lists.  A pass of at most 32 queries is served by a streaming kernel (each wave reads its own doc tiles from
 * memory into registers), a larger one by a 128 x 128 GEMM staged through LDS; the score bits are the same.
 *
 * srx_mx_score_docs: the contract of srx_dense_score_docs_half (cand_doc i32[nq][m] global ids, cand_count or NULL,
 * out_score f32[nq][m] every word written, padding / ids outside the corpus give +0.0f, duplicates legal); its bits equal
 * the search's at offset 0.  No workspace.
 *
 * ---- refusals -------------------------------------------------------------------------------------------------------------
 *
 * SRX_ERR_INVALID before anything touches a device, as sparse_rx_half.h lists them: a type outside srx_mx_type; dim_pad not a
 * multiple of 64 in [64, 1024]; convert: negative n_rows / row0 / n_total, row0 + n_rows > n_total, dim outside
 * [1, dim_pad], ld < dim, row0 % 32 != 0, more than 2^31 - 1 tiles in one call, and with n_rows > 0 a NULL emb / out, an emb
 * that is not 4-byte aligned, an out that is not 16-byte aligned; search: nq < 0, n_docs <= 0, k outside 1 .. 1024, a negative
 * doc_base or doc_base + n_docs >= 2^31 - 1, with nq > 0 a NULL pointer or a corpus / query block that is not 16-byte aligned,
 * and the filter rules of sparse_rx_filter.h; score_docs: nq < 0, m < 1, nq * m > 2^31 - 1, n_docs outside [1, 2^31 - 2], a
 * negative doc_base, with nq > 0 a NULL or misaligned pointer as above.  SRX_ERR_NOMEM: a NULL or too small workspace.
 * nq == 0 and n_rows == 0 return SRX_OK without a launch.
 */
#ifndef SPARSE_RX_MX_H
#define SPARSE_RX_MX_H

#include "sparse_rx.h"
#include "sparse_rx_filter.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum { SRX_MX_FP8 = 0, SRX_MX_FP4 = 1 } srx_mx_type;

int64_t srx_mx_bytes(int32_t type, int64_t n_rows, int32_t dim_pad);

int srx_mx_convert(int32_t device, int32_t type, const float *emb, int64_t ld, int64_t n_rows, int32_t dim, int32_t dim_pad, int64_t row0,
                   int64_t n_total, void *out, int32_t *flag, void *stream);

int64_t srx_mx_workspace_bytes(int32_t nq, int64_t n_docs, int32_t k);

int srx_mx_search(int32_t device, int32_t type, const void *corpus, int64_t n_docs, int32_t dim_pad, const float *queries, int32_t nq,
                  int32_t k, int64_t doc_base, const srx_doc_filter *filter /* NULL: none */, int32_t *out_doc, float *out_score,
                  int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream, float score_offset);

int srx_mx_score_docs(int32_t device, int32_t type, const void *corpus, int64_t n_docs, int32_t dim_pad, const float *queries, int32_t nq,
                      int64_t doc_base, const int32_t *cand_doc, const int32_t *cand_count, int32_t m, float *out_score, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_MX_H */
