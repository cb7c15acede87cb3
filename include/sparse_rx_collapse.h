/* sparse_rx_collapse.h -- field collapsing: at most n results per group of a ranked list, on the device.
 *
 * Tenth header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: every search, the fusion and the rerankers end in a ranked (doc, score, count) list per query.  The docs of a RAG
 * corpus are chunks of documents, and the top of such a list is routinely five chunks of one page.  sparse_rx_mmr.h answers
 * "near-copies"; this header answers the plainer request every passage-level retriever gets first: one, or at most n,
 * results per source document, author or thread (Elasticsearch `collapse`, Solr `group.limit`, Vespa `max(n)` per group).
 * The group key is a resident metadata column of sparse_rx_fields.h -- a parent id as an I64 column, a `source` category as
 * an I32 column of codes -- so the step needs no copy of the list to the host and no key lookup there.  The reference has no
 * grouping of results: nothing here replaces reference code.
 *
 * It is a step over a GIVEN list.  The top k of the collapsed COMPLETE ranking are the first k survivors of the complete
 * ranking, which a list of fixed depth may not contain; a caller that needs them pages the search (the search-after entry
 * point of sparse_rx.h) and collapses "kept so far ++ next page" -- legal because, for a list A that was not cut at k,
 * collapse(collapse(A) ++ B) == collapse(A ++ B).  That is why m goes up to two engine lists.
 *
 * ---- the contract -----------------------------------------------------------------------------------------------------
 *
 * Inputs       cand_doc i32[nq][m] GLOBAL doc ids, cand_score f32[nq][m], cand_count i32[nq] or NULL: the triple of any
 *              search, of the fusion or of the rerankers, unchanged, in ranking order.  1 <= m <= SRX_COLLAPSE_MAX_M = 2048,
 *              1 <= k <= m, 1 <= per_group <= INT32_MAX.
 * Column       `col` is ONE descriptor of sparse_rx_fields.h in HOST memory, type SRX_FIELD_I32 or SRX_FIELD_I64: a device
 *              array of n_docs values, naturally aligned, and optionally ONE filter row `valid` (16-byte aligned; bit d set =
 *              local doc d has a value; NULL = every doc has one).  Row i belongs to the doc with the global id doc_base + i.
 * Live         position c of query q is LIVE iff
 *                - c < min(max(cand_count[q], 0), m)   (a NULL cand_count means m), and
 *                - cand_doc[q][c] - doc_base, computed in 64 bits, is in [0, n_docs).
 *              Scores are never inspected, only copied: NaN payloads, negative scores and zeros pass through; there is no
 *              score > 0 rule.
 * Key          of a live position: the column's value at the local doc as int64 (an I32 value is widened).  A doc whose
 *              `valid` bit is 0 has NO key.
 * Group        of a live position with a key: all live positions of the list with the same int64 key.  Without a key:
 *                SRX_COLLAPSE_NULL_OWN   the position is a group of its own (it always survives);
 *                SRX_COLLAPSE_NULL_ONE   all keyless positions of the list form one group;
 *                SRX_COLLAPSE_NULL_DROP  the position is dropped.
 * Survivors    a live, not dropped position survives iff fewer than per_group EARLIER live positions of the list belong to
 *              its group.  The output is the first k survivors in list order: a subsequence of the input, the ranking is
 *              untouched.
 * Outputs      rows padded with -1 / +0.0f / -1 / 0; every word of every output row and every count is written.
 *                out_doc[q][t]         i32[nq][k]  the t-th survivor
 *                out_score[q][t]       f32[nq][k]  its score, the same bits as given
 *                out_count[q]          i32[nq]     min(k, survivors)
 *                out_pos[q][t]         i32[nq][k]  (may be NULL) the survivor's position in the input list, so that a caller
 *                                                  can carry other payload along
 *                out_group_size[q][t]  i32[nq][k]  (may be NULL) the live positions of the list in the survivor's group, itself
 *                                                  included ("7 more passages from this document").  It is relative to THE
 *                                                  LIST GIVEN, not to the corpus: a deeper list can report a larger group.
 *              The outputs must not overlap the inputs.
 * Execution    asynchronous on `stream`; allocates nothing, needs no workspace, uses no global atomics; ONE launch.
 *              nq == 0 returns SRX_OK without a launch.  The column, the validity row and the candidate arrays are only
 *              read; they must not be written while a call that uses them is in flight.
 * Precondition, NOT checked: no doc id twice in one list.  If one is, its two positions are simply two members of the
 *              group.
 *
 * Refused with SRX_ERR_INVALID before anything touches a device: a NULL col; a NULL col->data, or data misaligned for its
 * type (I32: 4 bytes, I64: 8); a type other than SRX_FIELD_I32 / SRX_FIELD_I64; a valid row that is not 16-byte aligned;
 * n_docs outside [1, 2^31 - 2] or a negative doc_base; m outside 1 .. 2048, k outside 1 .. m, per_group < 1; a null_policy
 * outside the enum; nq < 0 or nq * m > 2^31 - 1; with nq > 0 a NULL cand_doc, cand_score, out_doc, out_score or out_count.
 *
 * Not covered: F32 and SET64 columns (a float is no identity, a label set is not one key); ordering the groups by an
 * aggregate of their members (sum / mean of scores) or listing the members of a group contiguously -- the caller can
 * regroup k rows; a sharded index (columns are shard-local, as every filter row is); lists deeper than 2048.
 */
#ifndef SPARSE_RX_COLLAPSE_H
#define SPARSE_RX_COLLAPSE_H

#include "sparse_rx_fields.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SRX_COLLAPSE_NULL_OWN = 0, SRX_COLLAPSE_NULL_ONE = 1, SRX_COLLAPSE_NULL_DROP = 2 };
#define SRX_COLLAPSE_MAX_M 2048

int srx_collapse_topk(int32_t device,
                      const srx_field_col *col,  /* HOST struct of sparse_rx_fields.h: ONE column, type I32 or I64, optional valid row */
                      int64_t n_docs, int64_t doc_base,
                      const int32_t *cand_doc, const float *cand_score, const int32_t *cand_count /* may be NULL */,
                      int32_t nq, int32_t m, int32_t k, int32_t per_group, int32_t null_policy,
                      int32_t *out_doc, float *out_score, int32_t *out_count,
                      int32_t *out_pos /* may be NULL */, int32_t *out_group_size /* may be NULL */,
                      void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_COLLAPSE_H */
