/* sparse_rx_ivf.h -- IVF dense index: k-means lists over half-precision rows, probed and scanned by MFMA.
 *
 * Nineteenth header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: every other dense search of this library reads every row (or every code) for every call.  A clustered (inverted-file)
 * index partitions the corpus by k-means and reads, for a query, only the `nprobe` of `nlist` lists whose centroids score
 * highest: the bytes read fall by about nprobe / nlist with no change to the stored values.  The rows and the score chain are
 * those of sparse_rx_half.h, so the contract is exact: a search returns the exact top k of the PROBED lists with the half
 * index's own score bits, and with nprobe == nlist it equals srx_dense_search_half bit for bit.  No reference counterpart.
 *
 * ---- storage ----------------------------------------------------------------------------------------------------------
 *
 * There is no second copy of the rows.  The corpus is the fragment layout of sparse_rx_half.h with the rows PERMUTED so that
 * each list owns whole 32-row tiles: list c occupies tiles list_tile[c] .. list_tile[c + 1] - 1 (i32[nlist + 1],
 * list_tile[0] = 0, list_tile[nlist] = n_tiles), its members in ascending doc order, its last tile padded with zero rows; an
 * empty list has no tile.  row_doc i32[n_tiles * 32] is the shard-local doc of a packed row (-1: padding), doc_row i32[n_docs]
 * its inverse (not read by this library: it is the caller's map for srx_dense_score_docs_half over the permuted rows).  The
 * centroids are themselves a packed half corpus of nlist rows (ceil(nlist / 32) tiles), rounded like any row
 * (srx_dense_convert_half).  max_list_tiles >= the tiles of the largest list (a host value: it sizes the workspace; tiles of
 * a list beyond it are not scanned).  srx_ivf_desc is a HOST struct of device pointers.
 *
 * Limits: 1 <= nlist <= min(n_docs, 65536); dim_pad as the half index (a multiple of 64, <= 1024); 1 <= nprobe <=
 * min(nlist, 1024); 1 <= k <= 1024; n_docs in [1, 2^31 - 2].
 *
 * ---- scores -----------------------------------------------------------------------------------------------------------
 *
 * Every score of this header -- row against centroid, query against centroid, query against row -- is the fp32 accumulator of
 * ONE chain of v_mfma_f32_32x32x16_{f16,bf16} over the k-steps 0, 1, ..., dim_pad / 16 - 1 in ascending order from +0.0f, the
 * f32 side rounded to the index type as sparse_rx_half.h rounds queries: the bits are those of srx_dense_score_docs_half.
 * One kernel shape serves all three: a workgroup keeps 32 rows (or queries) as the A operand in LDS in fragment order
 * (32 * dim_pad halves, at most 64 KiB) and its four waves take alternate 32-row tiles of the B operand (centroids or a
 * list's rows) from memory, each tile read once per workgroup.
 *
 * ---- srx_ivf_assign ---------------------------------------------------------------------------------------------------
 *
 * rows f32[n][ld] (ld >= dim elements, 4-byte aligned).  out_list[i] = the centroid with the largest score, ties to the lowest
 * list id; no > 0 rule.  out_score f32[n] (or NULL) receives that score.  The arg-max is fused into the GEMM's epilogue: every
 * lane carries a running (score, list) pair per output row across the centroid tiles, one cross-lane reduction at the end; no
 * n x nlist matrix is written.  No workspace.
 *
 * ---- srx_ivf_update ---------------------------------------------------------------------------------------------------
 *
 * out_centroid f32[nlist][dim] from the F32 source rows (rows f32[.][ld]) and the member lists: member_ptr i64[nlist + 1],
 * member i32[member_ptr[nlist]] row numbers sorted by (list, row).  The order of every sum is the contract: per column, the
 * members of a list are taken in ascending order in chunks of 256; each chunk is summed sequentially from +0.0f; the chunk
 * partials are added sequentially in ascending chunk order from +0.0f; the result is divided by (float)count (IEEE division).
 * An empty list copies prev_centroid f32[nlist][dim] (out_centroid may be prev_centroid).  No atomics, no workspace.
 *
 * ---- srx_ivf_probe ----------------------------------------------------------------------------------------------------
 *
 * queries f32[nq][dim_pad], 16-byte aligned.  probe_list i32[nq][nprobe], probe_score f32[nq][nprobe]: the min(nprobe, nlist)
 * best centroids by (score descending, list ascending), no > 0 rule, rows padded with -1 / +0.0f.  The scores of a pass of at
 * most 1024 queries go to the workspace and a selection kernel cuts them.  A workspace of
 * srx_ivf_workspace_bytes(nq, nlist, nprobe, 1, 1) suffices.
 *
 * ---- srx_ivf_workspace_bytes(nq, nlist, nprobe, k, max_list_tiles) ----------------------------------------------------
 *
 * With r(x) = x rounded up to a multiple of 256, ldc = ceil(nlist / 32) * 32, S = max_list_tiles * 128 (the bytes of one
 * (query, list) score strip), P = min(nq, QB) queries per pass where QB = clamp(2^30 / (nprobe * S), 1, 1024),
 * N = P * nprobe pairs, fan = 4096 / k (integer), g = ceil(nprobe / fan):
 *
 *     r(min(nq, 1024) * ldc * 4)                probe scores
 *   + 4 * r(N * 4)                              probe list, probe score, cleaned list, pairs sorted by list
 *   + 4 * r((nlist + 1) * 4)                    per-list count, fill, pair offset, group offset
 *   + r(N * S)                                  score strips
 *   + 2 * r(N * k * 4) + r(N * 4)               candidate lists
 *   + (g > 1 ? 2 * (P * g * k * 8 + P * g * 4 + 256) : 0)      the merge's levels (srx_merge_workspace_bytes(P, nprobe, k))
 *   + 256.
 *
 * ---- srx_ivf_search ---------------------------------------------------------------------------------------------------
 *
 * The rules of srx_dense_search_half over the allowed docs OF THE PROBED LISTS: the ranked value is fl32(score +
 * score_offset), only values > 0 are results, order (value descending, doc ascending), ids doc_base + doc, padding -1 /
 * +0.0f, every word of every row and every count written.  `filter` (or NULL) has the semantics of sparse_rx_filter.h: rows
 * over the n_docs docs, tested on row_doc.  probe_list i32[nq][nprobe] (or NULL: computed as srx_ivf_probe does): entries
 * outside [0, nlist) (-1 is the padding) and duplicates of an earlier entry of the row are skipped.
 * Per pass: the (query, probed list) pairs are counting-sorted by list on the device; a work item is (list, a group of up to
 * 32 queries probing it): the group's queries are gathered as the A operand, the list's tiles stream from memory as B, each
 * read once per GROUP rather than once per query; the scores go to the pair's strip, a rank launch folds each strip into a
 * list of k, and the merge of this library joins a query's nprobe lists.  A batch of one query is the same kernels with one
 * live A row.  No workgroup waits for another: every loop is bounded by list_tile and stages are ordered by launches only.
 *
 * ---- refusals ---------------------------------------------------------------------------------------------------------
 *
 * SRX_ERR_INVALID before anything touches a device: a type outside srx_half_type; dim_pad not a multiple of 64 in
 * [64, 1024]; nlist outside [1, 65536]; assign: n outside [0, 2^31 - 1], dim outside [1, dim_pad], ld < dim, with n > 0 a
 * NULL centroids / rows / out_list, rows not 4-byte aligned, centroids not 16-byte aligned; update: dim outside [1, 1024],
 * ld < dim, a NULL pointer, rows not 4-byte aligned; a desc that is NULL or has nlist > n_docs, n_docs outside
 * [1, 2^31 - 2], n_tiles < 1 or > 2^26, max_list_tiles outside [1, n_tiles], a negative doc_base or doc_base + n_docs >=
 * 2^31 - 1, and with nq > 0 a NULL corpus / centroids / list_tile / row_doc or a corpus / centroids that is not 16-byte
 * aligned; probe and search: nq < 0, nprobe outside [1, min(nlist, 1024)], with nq > 0 a NULL or misaligned (16 bytes)
 * queries, NULL outputs; search: k outside [1, 1024] and the filter rules of sparse_rx_filter.h; workspace_bytes: nq < 0 or
 * any other argument < 1, nlist > 65536, nprobe > min(nlist, 1024), k > 1024.  SRX_ERR_NOMEM: a NULL or too small workspace.
 * nq == 0 and n == 0 return SRX_OK without a launch.
 */
#ifndef SPARSE_RX_IVF_H
#define SPARSE_RX_IVF_H

#include "sparse_rx.h"
#include "sparse_rx_filter.h"
#include "sparse_rx_half.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct srx_ivf_desc {
    int32_t device, type;         /* srx_half_type */
    int64_t n_docs, doc_base;
    int64_t n_tiles;              /* 32-row tiles of the permuted corpus */
    int64_t max_list_tiles;
    int32_t dim_pad, nlist;
    const void *corpus;           /* device, fragment order, n_tiles tiles */
    const void *centroids;        /* device, fragment order, ceil(nlist / 32) tiles */
    const int32_t *list_tile;     /* device, i32[nlist + 1] */
    const int32_t *row_doc;       /* device, i32[n_tiles * 32] */
    const int32_t *doc_row;       /* device, i32[n_docs]; not read by the library */
} srx_ivf_desc;

int srx_ivf_assign(int32_t device, int32_t type, const void *centroids_packed, int32_t nlist, int32_t dim, int32_t dim_pad,
                   const float *rows, int64_t ld, int64_t n, int32_t *out_list, float *out_score /* NULL: not wanted */, void *stream);

int srx_ivf_update(int32_t device, const float *rows, int64_t ld, int32_t dim, int32_t nlist, const int64_t *member_ptr,
                   const int32_t *member, const float *prev_centroid, float *out_centroid, void *stream);

int srx_ivf_probe(const srx_ivf_desc *desc, const float *queries, int32_t nq, int32_t nprobe, int32_t *probe_list, float *probe_score,
                  void *workspace, int64_t workspace_bytes, void *stream);

int64_t srx_ivf_workspace_bytes(int32_t nq, int32_t nlist, int32_t nprobe, int32_t k, int64_t max_list_tiles);

int srx_ivf_search(const srx_ivf_desc *desc, const float *queries, int32_t nq, int32_t nprobe, int32_t k,
                   const int32_t *probe_list /* NULL: computed */, const srx_doc_filter *filter /* NULL: none */, int32_t *out_doc,
                   float *out_score, int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream, float score_offset);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_IVF_H */
