/* sparse_rx_graph.h -- graph dense index: a fixed-degree neighbour graph over half-precision rows, walked by a beam search.
 *
 * Twenty-second header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: the IVF, PQ and IVF-PQ indexes cut a query down to lists chosen by coarse centroids; at the nprobe a recall near 1 needs,
 * a large batch re-reads most of the corpus, and one query pays for ten short launches.  A neighbour graph (HNSW; on GPUs the
 * fixed-degree CAGRA form) touches a few thousand rows per query whatever the corpus size, in ONE launch, needs no permuted copy
 * of the rows and keeps the score bits of sparse_rx_half.h.  No reference counterpart.
 *
 * ---- storage ----------------------------------------------------------------------------------------------------------
 *
 * No second copy of the rows and no permutation: `corpus` is exactly the buffer srx_dense_convert_half writes (fragment order,
 * sparse_rx_half.h).  `graph` is i32[n_docs][degree], row-major: shard-local row numbers, padded with -1; degree is 16, 32 or 64.
 * srx_graph_desc is a HOST struct of device pointers.  n_docs in [1, 2^31 - 2]; dim_pad as the half index.
 *
 * ---- srx_graph_search -------------------------------------------------------------------------------------------------
 *
 * One launch, no workspace; one workgroup serves one query, every loop is bounded by an argument, no workgroup waits for another.
 *   itopk     L, the beam width: a multiple of 32 in [32, 512]
 *   width     p, parents per step: [1, 8], p * degree <= 512
 *   max_iter  T: [1, 1024]
 *   seed_doc  i32[nq][n_seed] GLOBAL ids, or NULL; n_seed in [1, 512]
 *   k         [1, L]
 *   filter, score_offset   as srx_dense_search_half
 *   out_stat  i32[nq][2] or NULL: the steps run, the docs scored
 *   n_seed + T * p * degree <= 8192: the visit budget (it sizes the visited table in LDS).
 *
 * The contract is exact (tests/graph_ref.py restates it).  v(d) = fl32(score(q, d) + score_offset), score with the bits of
 * srx_dense_score_docs_half: one ascending chain of v_mfma_f32_32x32x16_{f16,bf16} from +0.0f, the query rounded as that call
 * rounds it.  Entries are ordered by (v descending, doc ascending).  For one query:
 *   1. Seeds.  With seed_doc NULL seed j is row floor(j * n_docs / n_seed) (64-bit arithmetic), the same for every query;
 *      otherwise the given ids, those outside [doc_base, doc_base + n_docs) and repeats skipped.  The distinct seeds are scored
 *      and marked visited; the beam is their best L entries, all unexpanded.
 *   2. Steps, up to T times.  The parents are the first at most p unexpanded entries of the beam in beam order; none: stop;
 *      otherwise they are marked expanded.  The new docs are the distinct entries of the parents' graph rows that lie in
 *      [0, n_docs) and are not visited (anything else, -1 included, is skipped: a graph of arbitrary contents reads nothing out
 *      of bounds).  They are scored and marked visited; the beam becomes the best L of (beam U new), entries keeping their
 *      expanded flag.
 *   3. Result.  The beam's entries in order, those the filter allows whose v > 0, the first k of them, as ids doc_base + row;
 *      rows padded with -1 / +0.0f; every word of every row and every count written.  The walk itself ignores the filter: a
 *      forbidden doc is a stepping stone.
 * The visited set is exact (every doc ever scored for the query) and the beam after a step is the top L of a set under a total
 * order, so the result does not depend on launch geometry, wave timing, nq or a query's position in the batch.  Queries with
 * non-finite values are unspecified, as in sparse_rx_half.h.
 *
 * ---- srx_graph_prune --------------------------------------------------------------------------------------------------
 *
 * The CAGRA rank rule, integers only.  knn i32[n][d0], local ids, best first; d0 in [degree, 128].  An entry of row x is invalid
 * if it is outside [0, n), equals x, or repeats an earlier entry of the row.  For a valid entry y_j at position j,
 * detours(j) = the number of valid positions i < j for which knn[y_i][r] == y_j at some position r < j (each i counts at most
 * once).  out i32[n][degree]: the valid positions with the smallest (detours, j), in that order, padded with -1.  No workspace.
 *
 * ---- srx_graph_merge --------------------------------------------------------------------------------------------------
 *
 * Adds reverse edges.  fwd i32[n][degree] (the pruned graph); the reverse lists as a CSR: rev_ptr i64[n + 1] (ascending, a
 * precondition), rev_src i32[rev_ptr[n]], the sources of the edges into each node ordered by (position of the node in the
 * source's row, source).  out[y] = the first `degree` distinct valid ids (inside [0, n) and not y) of the sequence
 * fwd[y][0 : degree/2], rev[y][0 : degree/2], fwd[y][degree/2 : degree], padded with -1.  One wave serves one node.
 *
 * ---- refusals ---------------------------------------------------------------------------------------------------------
 *
 * SRX_ERR_INVALID before anything touches a device: a NULL desc; a type outside srx_half_type; dim_pad not a multiple of 64 in
 * [64, 1024]; degree outside {16, 32, 64}; n_docs outside [1, 2^31 - 2]; a negative doc_base or doc_base + n_docs >= 2^31 - 1;
 * nq < 0; itopk, width, max_iter, n_seed, k or the visit budget outside the ranges above; with nq > 0 a NULL corpus / graph /
 * queries / output, a corpus or query block that is not 16-byte aligned, a graph or seed_doc that is not 4-byte aligned; the
 * filter rules of sparse_rx_filter.h; prune and merge: n outside [0, 2^31 - 2], a bad degree, d0 outside [degree, 128], with
 * n > 0 a NULL or misaligned (4 bytes; rev_ptr 8) pointer.  nq == 0 and n == 0 return SRX_OK without a launch.
 */
#ifndef SPARSE_RX_GRAPH_H
#define SPARSE_RX_GRAPH_H

#include "sparse_rx.h"
#include "sparse_rx_filter.h"
#include "sparse_rx_half.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct srx_graph_desc {
    int32_t device, type;         /* srx_half_type */
    int64_t n_docs, doc_base;
    int32_t dim_pad, degree;
    const void *corpus;           /* device, fragment order, ceil(n_docs / 32) tiles */
    const int32_t *graph;         /* device, i32[n_docs][degree] */
} srx_graph_desc;

int srx_graph_search(const srx_graph_desc *desc, const float *queries, int32_t nq, int32_t itopk, int32_t width, int32_t max_iter,
                     const int32_t *seed_doc /* NULL: spread rows */, int32_t n_seed, int32_t k, const srx_doc_filter *filter /* NULL: none */,
                     int32_t *out_doc, float *out_score, int32_t *out_count, int32_t *out_stat /* NULL: not wanted */, void *stream,
                     float score_offset);

int srx_graph_prune(int32_t device, const int32_t *knn, int64_t n, int32_t d0, int32_t degree, int32_t *out, void *stream);

int srx_graph_merge(int32_t device, const int32_t *fwd, int64_t n, int32_t degree, const int64_t *rev_ptr, const int32_t *rev_src,
                    int32_t *out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_GRAPH_H */
