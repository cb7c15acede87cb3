/* sparse_rx_ivfpq.h -- IVF-PQ dense index: 8-bit product codes of the residual x - centroid, kept in k-means lists.
 *
 * Twenty-first header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h; every refusal happens before anything
 * touches a device; asynchronous on `stream`; nothing is allocated).
 *
 * Why: sparse_rx_ivf.h reads only nprobe of nlist lists but keeps every half row resident; sparse_rx_pq.h keeps 96 bytes per
 * 768-dim row but reads every code for every query.  This header joins them: the coarse quantiser and the lists of the first,
 * the codes, the table and the per-row sum of the second -- of the RESIDUAL of a row against the rounded centroid of its list.
 * No reference counterpart.
 *
 * ---- storage ----------------------------------------------------------------------------------------------------------
 *
 * srx_ivfpq_desc is a HOST struct of device pointers.
 *   centroids   the nlist centroids as a packed half corpus (f16 or bf16; ceil(nlist / 32) tiles in the fragment order of
 *               sparse_rx_half.h), exactly as in srx_ivf_desc.  Rows are assigned with srx_ivf_assign.
 *   codes       the tiled layout of sparse_rx_pq.h (64-row tiles of 16-byte pieces, M_pad = M rounded up to 16) with the rows
 *               PERMUTED so that list c owns the whole tiles list_tile[c] .. list_tile[c + 1] - 1 (i32[nlist + 1], list_tile[0] = 0,
 *               list_tile[nlist] = n_tiles): its members in ascending doc order, its last tile padded with zero codes; an empty
 *               list has no tile.
 *   maps        row_doc i32[n_tiles * 64]: the shard-local doc of a packed row (-1: padding); doc_row i32[n_docs]: its inverse;
 *               tile_list i32[n_tiles]: the list that owns a tile.
 *   codebooks   the residual codebooks f32[M][256][dsub], 16-byte aligned.
 *   max_list_tiles  a host value >= the tiles of the largest list: it sizes the workspace; tiles of a list beyond it are not scanned.
 *
 * Limits (those of both parent headers): dsub in {4, 8, 16}; 1 <= dim <= 1024; M = ceil(dim / dsub) <= 128; dim_pad = dim rounded
 * up to a multiple of 64; 1 <= nlist <= min(n_docs, 65536); 1 <= nprobe <= min(nlist, 1024); 1 <= k <= 1024; n_docs in
 * [1, 2^31 - 2]; 1 <= n_tiles <= 2^25.
 *
 * ---- arithmetic (the contract) ----------------------------------------------------------------------------------------
 *
 * There is no tolerance.  Every fp32 operation below is rounded on its own (no FMA); fl() is that rounding.
 *
 *   residual  r[j] = fl(x[j] - c[j]) for j < dim, where c[j] is the f32 value of the ROUNDED centroid of the row's list (the half
 *             value the packed centroids hold); columns dim .. M * dsub - 1 are zeros.
 *   code      the encode rule of sparse_rx_pq.h applied to r with the residual codebooks (ties to the lowest code).
 *   table     LUT[q][m][c]: the table rule of srx_pq_lut on the f32 query with the residual codebooks.  One table per query
 *             serves every list: the metric is the inner product, so q . x ~ q . c + q . r.
 *   coarse    coarse[q][c] has the bits srx_ivf_probe and srx_dense_score_docs_half give for query q against centroid row c
 *             (one MFMA chain over dim_pad / 16 k-steps from +0.0f, the query rounded to the centroids' type).
 *   score     score[q][d] = fl(coarse[q][list(d)] + s), s = the sequential fp32 sum from +0.0f over m = 0 .. M - 1 ascending
 *             of LUT[q][m][code[d][m]].
 *   ranking   the rules of srx_ivf_search over the allowed docs of the probed lists: the value is fl(score + score_offset),
 *             only values > 0 are results, order (value descending, doc ascending), ids doc_base + doc, padding -1 / +0.0f,
 *             every word of every row and every count written.  A filter's rows are over the n_docs docs and are tested on
 *             row_doc.  In probe_list, -1, entries outside [0, nlist) and repeats of an earlier entry of the row are skipped.
 *
 * The bits of a (query, doc) pair do not depend on nq, k, nprobe, the filter, the launch geometry or the entry point.
 *
 * ---- srx_ivfpq_encode -------------------------------------------------------------------------------------------------
 *
 * The residual encoder for a CHUNK of packed rows row0 .. row0 + n_rows - 1 of the n_total = n_tiles * 64 packed rows
 * (row0 % 64 == 0).  Packed row row0 + i takes source row src_row[i] of x (f32[n_src][ld], ld >= dim elements; -1 or a value
 * outside [0, n_src): padding, zero codes) and belongs to list row_list[i].  A call writes every 16-byte piece of the 64-row
 * tiles it covers (zeros for the rows of its last tile it does not hold and for bytes M .. M_pad - 1).  The kernel is the PQ
 * encoder with the gather and the centroid subtraction in front: a subspace's codebook in LDS, a lane owns a row, four distance
 * chains in flight.
 *
 * ---- srx_ivfpq_search -------------------------------------------------------------------------------------------------
 *
 * queries f32[nq][dim_pad] (columns dim .. dim_pad - 1 zeros), 16-byte aligned: one buffer feeds the probe and the table.
 * probe_list i32[nq][nprobe] or NULL (computed as srx_ivf_probe does).
 *
 * Per pass of P queries: the probe writes every centroid's score; srx_pq_lut's kernel writes LUT[P][M][256]; one short launch
 * per query cleans its probe row and leaves, beside the table, the start tile, the coarse term and the running tile count
 * (a prefix sum over at most 1024 list lengths) of each slot.  The scan's work item is (query, slice): the tiles of the
 * query's probed lists, concatenated in probe order, are cut into S slices of equal tile count, so a slice boundary may fall
 * inside a list and work stays balanced when lists are skewed.  The workgroup copies its query's table into LDS once (M KiB);
 * its waves take alternate tiles of the slice; a lane owns one row, whose pieces stay in registers; the next tile's loads are
 * issued before this tile's sums, across list boundaries too; per subspace one byte extract, one LDS read, one add; the coarse
 * term is wave-uniform per tile.  Scores go to the (query, slice) strip, a rank launch folds each strip into a list of k
 * (filter on row_doc, offset, > 0), the merge of this library joins a query's S lists.  No workgroup waits for another: every
 * loop is bounded by list_tile clamped to n_tiles and max_list_tiles, stages are ordered by launches only.
 *
 * The plan, with T = nprobe * max_list_tiles (the most tiles a query reads) and integer divisions:
 *     P  = min(nq, QB), QB = clamp(2^30 / (256 T), 1, 1024)          queries per pass
 *     S  = max(1, min(512 / P, 64, (T + 15) / 16))                   slices per query: P * S fills the machine for small
 *                                                                    batches, S = 1 from 512 queries up
 *     L  = ceil(T / S)                                               tiles a slice holds at most
 *
 * srx_ivfpq_workspace_bytes(nq, nlist, nprobe, k, M, max_list_tiles), with r(x) = x rounded up to a multiple of 256,
 * ldc = ceil(nlist / 32) * 32 and N = P * nprobe:
 *
 *     r(4 P ldc)                          every centroid's score
 *   + r(1024 P M)                         the tables
 *   + 4 r(4 N) + r(4 P (nprobe + 1))      probe list, probe score, start tile, coarse term; running tile counts
 *   + r(256 P S L) + r(4 P S L)           score strips, the packed tile of each strip tile
 *   + 2 r(4 P S k) + r(4 P S)             candidate lists
 *   + srx_merge_workspace_bytes(P, S, k)  the merge's levels (0 while S * k <= 4096)
 *   + 256.
 *
 * ---- srx_ivfpq_score_docs ---------------------------------------------------------------------------------------------
 *
 * The candidate contract of srx_pq_score_docs: cand_doc i32[nq][m] GLOBAL ids, cand_count i32[nq] or NULL, out_score f32[nq][m]
 * with every word written; padding (-1, entries at or beyond cand_count[q]) and ids outside [doc_base, doc_base + n_docs) give
 * +0.0f; duplicates are legal; nq * m <= 2^31 - 1.  No offset and no > 0 rule: the bits are those of the search at
 * score_offset 0.  The route is doc -> doc_row -> tile_list, then the coarse term through srx_dense_score_docs_half over the
 * centroid corpus, then the code sum in the search's order.  The workspace holds the list of every candidate:
 * srx_ivfpq_score_docs_workspace_bytes(nq, m) = r(4 nq m) + 256.
 *
 * ---- refusals ---------------------------------------------------------------------------------------------------------
 *
 * SRX_ERR_INVALID before anything touches a device: a type outside srx_half_type; dsub outside {4, 8, 16}; dim outside
 * 1 .. 1024; M > 128; dim_pad other than dim rounded up to a multiple of 64; nlist outside [1, 65536];
 * encode: negative n_src / n_rows / row0 / n_total, row0 + n_rows > n_total, row0 % 64 != 0, ld < dim, more than 2^31 - 1 rows in
 * one call, and with n_rows > 0 a NULL pointer, an x that is not 4-byte aligned, centroids / codebooks / out_codes that are not
 * 16-byte aligned;
 * a desc that is NULL or has nlist > n_docs, n_docs outside [1, 2^31 - 2], n_tiles outside [1, 2^25], max_list_tiles outside
 * [1, n_tiles], a negative doc_base or doc_base + n_docs >= 2^31 - 1, and with nq > 0 a NULL codes / codebooks / centroids /
 * list_tile / row_doc / doc_row / tile_list or codes / codebooks / centroids that are not 16-byte aligned;
 * search: nq < 0, nprobe outside [1, min(nlist, 1024)], k outside [1, 1024], nprobe * max_list_tiles > 2^26 (workspace_bytes too),
 * the filter rules of sparse_rx_filter.h, with nq > 0 a NULL or misaligned (16 bytes) queries, NULL outputs; score_docs: nq < 0, m < 1, nq * m > 2^31 - 1, with nq > 0 a NULL or
 * misaligned queries, a NULL cand_doc / out_score; workspace_bytes: nq < 0, nlist outside [1, 65536], nprobe outside
 * [1, min(nlist, 1024)], k outside [1, 1024], M outside [1, 128], max_list_tiles outside [1, 2^25];
 * score_docs_workspace_bytes: nq < 0, m < 1, nq * m > 2^31 - 1.  SRX_ERR_NOMEM: a NULL or too small workspace.  nq == 0 and
 * n_rows == 0 return SRX_OK without a launch.
 */
#ifndef SPARSE_RX_IVFPQ_H
#define SPARSE_RX_IVFPQ_H

#include "sparse_rx.h"
#include "sparse_rx_filter.h"
#include "sparse_rx_half.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct srx_ivfpq_desc {
    int32_t device, type;         /* srx_half_type of the centroids */
    int64_t n_docs, doc_base;
    int64_t n_tiles;              /* 64-row tiles of the permuted codes */
    int64_t max_list_tiles;
    int32_t dim, dsub, dim_pad, nlist;
    const void *codes;            /* device, tiled, n_tiles tiles */
    const float *codebooks;       /* device, f32[M][256][dsub] */
    const void *centroids;        /* device, fragment order, ceil(nlist / 32) tiles */
    const int32_t *list_tile;     /* device, i32[nlist + 1] */
    const int32_t *row_doc;       /* device, i32[n_tiles * 64] */
    const int32_t *doc_row;       /* device, i32[n_docs] */
    const int32_t *tile_list;     /* device, i32[n_tiles] */
} srx_ivfpq_desc;

int srx_ivfpq_encode(int32_t device, int32_t type, const void *centroids_packed, int32_t nlist, int32_t dim_pad, const float *x, int64_t ld,
                     int64_t n_src, int32_t dim, int32_t dsub, const float *codebooks, const int32_t *src_row, const int32_t *row_list,
                     int64_t n_rows, int64_t row0, int64_t n_total, void *out_codes, void *stream);

int64_t srx_ivfpq_workspace_bytes(int32_t nq, int32_t nlist, int32_t nprobe, int32_t k, int32_t M, int64_t max_list_tiles);

int srx_ivfpq_search(const srx_ivfpq_desc *desc, const float *queries, int32_t nq, int32_t nprobe, int32_t k,
                     const int32_t *probe_list /* NULL: computed */, const srx_doc_filter *filter /* NULL: none */, int32_t *out_doc,
                     float *out_score, int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream, float score_offset);

int64_t srx_ivfpq_score_docs_workspace_bytes(int32_t nq, int32_t m);

int srx_ivfpq_score_docs(const srx_ivfpq_desc *desc, const float *queries, int32_t nq, const int32_t *cand_doc, const int32_t *cand_count,
                         int32_t m, float *out_score, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_IVFPQ_H */
