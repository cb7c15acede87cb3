/* sparse_rx_quant.h -- dense index build on the device: quantise embeddings and query vectors.
 *
 * Third header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: the dense searches of sparse_rx.h take INT8 / uint8 codes and scale tables; an encoder leaves f32 vectors on the
 * device.  The four entry points below are the reference's quantisers (rag_system/core/retriever_registry.py:435-462 for
 * a corpus, :482-491 for a query, :555 for the de-quantised uint8 query) as HIP kernels, so neither a corpus nor a query
 * batch travels through the host.  The reference's arithmetic is plain fp32 NumPy; the kernels repeat it operation by
 * operation, so codes and scales are the reference's bit for bit.
 *
 * Every call is asynchronous on `stream`, allocates nothing and needs no workspace.  All pointers are device pointers.
 *
 * Inputs
 *   emb / q     f32 rows with a row stride of ld >= dim ELEMENTS.  4-byte alignment is enough (a column slice of a wider
 *               tensor is a legal input); with a 16-byte aligned base, ld % 4 == 0 and dim % 4 == 0 the rows are read
 *               with 16-byte loads.
 *   dim, dim_pad  1 <= dim <= dim_pad <= 1024.  i8: dim_pad is one of the INT8 engine's row lengths (32, 64, 96, 128,
 *               192, 256, 384, 512, 768, 1024).  u8: dim_pad is a multiple of 64.  Columns dim .. dim_pad - 1 of every
 *               output row are written as zeros: code 0 and out_deq +0.0f (not the row's minimum).
 *   flag        i32[1] or NULL, zeroed by the caller.  See "Where the reference is undefined".
 *
 * Corpus calls quantise a CHUNK: emb holds rows row0 .. row0 + n_rows - 1 of a corpus of n_total rows, while out_corpus
 * and out_scale[s] are the buffers of the WHOLE corpus -- a host matrix can be streamed through a small staging tensor.
 *   i8, packed = 0   out_corpus is i8[n_total][dim_pad].
 *   i8, packed = 1   out_corpus is the srx_dense_packed_bytes of (n_total, dim_pad), in exactly the fragment
 *                    order srx_dense_pack_i8 writes (sparse_rx.h); no row-major intermediate exists.  row0 must be a multiple
 *                    of 32.  A call writes every byte of the 32-row tiles it covers: zeros for the rows of its last
 *                    tile it does not hold (rows >= n_total of the corpus' last tile among them), so only the chunk
 *                    that ends the corpus may end inside a tile.
 *   out_scale        f32[n_total]: the scale of row r at [r].
 *   u8               out_corpus is u8[n_total][dim_pad]; out_scales is f32[2 n_total], the scale of row r at [r] and its
 *                    minimum at [n_total + r]: the reference writer's table (:459), as srx_dense_search_u8 takes it.
 * Query calls: out_q is i8 / u8 [nq][dim_pad]; i8: out_scale f32[nq]; u8: out_scales f32[nq][2] = {scale, min} and
 *   out_deq f32[nq][dim_pad], the de-quantised block srx_dense_search_u8 takes.  out_q and out_scales of the u8 call may
 *   be NULL when only out_deq is wanted.
 *
 * Arithmetic: fp32, every operation rounded on its own, IEEE division, denormals kept, rintf = round to nearest even
 * (np.round):
 *   i8 row     m = max_i |x_i|; s = max(m, 1e-8f); code_i = (int8) rintf((x_i / s) * 127.0f); out_scale = s.
 *   i8 query   s = max_i |x_i|; the same code expression; out_scale = s / 127.0f.
 *   u8 row     mn, mx over the row; sc = max((mx - mn) / 255.0f, 1e-8f); code_i = (uint8) rintf((x_i - mn) / sc).
 *   u8 query   sc = (mx - mn) / 255.0f, no clamp; the same code; out_scales[q] = {sc, mn};
 *              out_deq[q][i] = (float)code_i * sc + mn (two roundings).
 *
 * Where the reference is undefined (it divides by zero or casts NaN) the result is defined here and a bit is ORed into
 * *flag (one vector atomic per wave that saw such a row; nothing is written to flag otherwise):
 *   bit 0 (SRX_QUANT_NONFINITE)   a row or query holds a non-finite value, or its mx - mn overflows.  Codes are 0; an i8
 *         row gets scale 1e-8f, a u8 row scale 1e-8f and min 0, a query scale 0 (u8: scale 0, min 0, out_deq 0).
 *   bit 1 (SRX_QUANT_DEGENERATE)  queries only.  An all-zero i8 query: codes 0, scale 0 (every score is 0).  A u8 query
 *         whose sc is 0 (a constant query; also a spread too small for sc to be a nonzero float): codes 0, scale 0,
 *         min = mn, so out_deq = 0.0f * 0.0f + mn, the value itself.
 *   An all-zero or constant corpus ROW is not degenerate: the 1e-8f clamp handles it as the reference does.
 *   Not specified: the sign of a stored minimum that is a zero when both +0 and -0 occur in the row.
 *
 * Refused with SRX_ERR_INVALID before anything touches a device: negative n_rows / row0 / n_total / nq;
 * row0 + n_rows > n_total; dim, dim_pad or ld out of range; a dim_pad the form does not take; packed other than 0 / 1;
 * row0 % 32 != 0 with packed; more than 2^31 - 1 tiles of 32 rows in one call; and, with a count above 0, a NULL emb / q,
 * out_corpus, out_scale[s] (i8 query: out_q, out_scale; u8 query: out_deq), an input that is not 4-byte aligned and a
 * code or out_deq output that is not 16-byte aligned.  n_rows == 0 / nq == 0 returns SRX_OK without a launch.
 */
#ifndef SPARSE_RX_QUANT_H
#define SPARSE_RX_QUANT_H

#include "sparse_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRX_QUANT_NONFINITE 1  /* flag bit 0 */
#define SRX_QUANT_DEGENERATE 2 /* flag bit 1 */

int srx_dense_quantize_i8(int32_t device, const float *emb, int64_t ld, int64_t n_rows, int32_t dim, int32_t dim_pad,
                          int64_t row0, int64_t n_total, int32_t packed, void *out_corpus, float *out_scale,
                          int32_t *flag, void *stream);

int srx_dense_quantize_u8(int32_t device, const float *emb, int64_t ld, int64_t n_rows, int32_t dim, int32_t dim_pad,
                          int64_t row0, int64_t n_total, uint8_t *out_corpus, float *out_scales, int32_t *flag, void *stream);

int srx_dense_quantize_queries_i8(int32_t device, const float *q, int64_t ld, int32_t nq, int32_t dim, int32_t dim_pad,
                                  int8_t *out_q, float *out_scale, int32_t *flag, void *stream);

int srx_dense_quantize_queries_u8(int32_t device, const float *q, int64_t ld, int32_t nq, int32_t dim, int32_t dim_pad,
                                  uint8_t *out_q, float *out_scales, float *out_deq, int32_t *flag, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_QUANT_H */
