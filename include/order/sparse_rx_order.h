/* sparse_rx_order.h -- order by a field: the first k docs of a filter row, or of a result list, by the value a metadata column
 * holds for them, on the device.
 *
 * Thirteenth header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: every search of this library ranks by relevance.  "Newest first", "cheapest first", a time-ordered feed that pages
 * forward (Elasticsearch `sort` + `search_after`, Solr `sort` + `cursorMark`, Qdrant `order_by`) needed a filter row copied
 * to the host and a second copy of the metadata walked there.  Sorting the BM25 top-k by date is something else: the newest
 * matching doc is usually not among the most relevant 1 024.  The columns of sparse_rx_fields.h are resident and every doc
 * set is a row of sparse_rx_filter.h: this header selects over them where they are.  The reference has no field ordering:
 * nothing here replaces reference code.
 *
 * ---- the contract -----------------------------------------------------------------------------------------------------
 *
 * Column       `col` is ONE descriptor of sparse_rx_fields.h in HOST memory, of type I32, I64 or F32 (a SET64 column is
 *              refused: a label set has no order): a device array of n_docs values, naturally aligned (I32 / F32: 4 bytes,
 *              I64: 8), and optionally ONE filter row `valid` (16-byte aligned; bit d set = local doc d has a value; NULL =
 *              every doc has one).  Row i of the column belongs to the doc with the global id doc_base + i.
 * Value        a doc HAS a value when its `valid` bit is set (or `valid` is NULL) and, for F32, the value is not NaN: a NaN
 *              is "no value", as it is "in no bin" for sparse_rx_facets.h.  Integers compare as signed int64 (I32 widened).
 *              F32 compares by IEEE, -0 == +0.
 * Order        of one call.  For two docs a, b of the index, a PRECEDES b:
 *                both have a value    the smaller value precedes under SRX_ORDER_ASC, the larger under SRX_ORDER_DESC; on
 *                                     equal values the smaller doc id precedes, in BOTH directions;
 *                both lack a value    the smaller doc id precedes;
 *                exactly one has one  the valued doc precedes under NULLS_LAST and NULLS_DROP, the valueless doc under
 *                                     NULLS_FIRST.
 *              A strict total order over the docs of the index; it depends on no row.
 * Doc set      srx_order_topk, row r: read exactly as srx_facet_counts reads its row -- a NULL `filter` means every doc; a NULL
 *              filter->q_filter means row 0; otherwise the row is q_filter[r] (i32[n_rows]), and -1 means every doc.  Only
 *              local docs 0 <= d < n_docs belong, whatever bits are set above.  Under NULLS_DROP the valueless docs are
 *              removed from the set.
 * Cursor       after_doc[r] (device i32[n_rows], GLOBAL ids; a NULL after_doc = no cursor for any row):
 *                -1                                            no cursor;
 *                another id outside [doc_base, doc_base + n_docs)   the row's result is EMPTY (`total` is still counted);
 *                a doc c of the index                          only the docs of the set that c strictly precedes stay.
 *              The kernel reads c's value from the column itself: c need not be in the set.  A valueless c under NULLS_DROP
 *              therefore gives an empty result.  Paging is stateless: the next page's cursor is this page's last doc id.
 * Outputs      srx_order_topk: out_doc i32[n_rows][k] holds the first min(k, remaining) docs of the set after the cursor, in
 *              the order above, as GLOBAL ids; 1 <= k <= 1024 (SRX_MAX_K).  out_key i64[n_rows][k] holds the value as int64
 *              (I32 widened; F32: the float's stored bits in the low 32, zero-extended, so -0 stays -0; a valueless doc: 0).
 *              out_extra i32[n_rows][3] = {count, valued, total}:
 *                count   entries written for the row;
 *                valued  how many of them have a value -- the valueless entries are contiguous, the last count - valued
 *                        under NULLS_LAST and the first count - valued under NULLS_FIRST;
 *                total   docs of the row's set BEFORE NULLS_DROP and before the cursor: the "total hits".
 *              Rows are padded with -1 (doc) and 0 (key).  Every word of every output is written; a second call into the same
 *              buffers gives the same result.  The outputs and the workspace must not overlap the inputs or each other.
 * Lists        srx_order_lists, list q: the LIVE positions are those of srx_collapse_topk, word for word -- position c is
 *              live iff c < min(max(cand_count[q], 0), m) (a NULL cand_count means m) and cand_doc[q][c] - doc_base, computed
 *              in 64 bits, is in [0, n_docs).  1 <= m <= 2048 (SRX_ORDER_MAX_M), 1 <= k <= m, nq * m <= 2^31 - 1.  The live
 *              positions are STABLY sorted by the value order above; the tie-break -- between equal values and between
 *              valueless positions -- is the position in the list, not the doc id: docs of one day keep their relevance order.
 *              Valueless positions go last, first, or are dropped.  The first k of that order are written: out_doc the doc,
 *              out_score the bits of cand_score at that position (copied, never inspected), out_key as above, out_pos
 *              (optional, may be NULL) the position in the input, out_extra i32[nq][3] = {count, valued, live} with `live`
 *              the number of live positions before NULLS_DROP.  Rows are padded with -1 / +0.0f / 0 / -1.  A doc id that
 *              occurs twice stays twice.  One launch, no workspace.
 * Workspace    srx_order_topk only.  srx_order_workspace_bytes is a pure host function:
 *                seg_docs = 8192 * ceil(max(32768, 64 * k) / 8192)      docs one workgroup scans for one row
 *                segments = ceil(n_docs / seg_docs)
 *                bytes    = n_rows * segments * (12 * k + 8)            per (row, segment): k ranks of 96 bits, {kept, total}
 *              (0 for n_rows == 0; a negative value for arguments the call would refuse: n_docs outside [1, 2^31 - 2],
 *              n_rows < 0, k outside [1, 1024], n_rows * k > 2^31 - 1).  A row's merge input is at most n_docs / 64 ranks.
 *              The workspace must be 8-byte aligned; a shorter one is refused with SRX_ERR_NOMEM.  Its content is scratch.
 * Execution    asynchronous on `stream`; allocates nothing.  srx_order_topk is two launches (scan, merge), srx_order_lists
 *              one.  Integer work only, no global atomics: the result is exact and independent of the launch geometry.
 *              n_rows == 0 / nq == 0 returns SRX_OK without a launch.  The column, the validity row, the filter rows, the
 *              cursors and the candidate arrays are only read; they must not be written while a call that uses them is in
 *              flight.
 *
 * Refused with SRX_ERR_INVALID before anything touches a device: a NULL col; a NULL col->data, or data misaligned for its
 * type; a SET64 or unknown column type; a valid row that is not 16-byte aligned; `order` or `nulls` outside its enum; n_docs
 * outside [1, 2^31 - 2]; a negative doc_base, or one with doc_base + n_docs >= 2^31 - 1; k outside [1, 1024] (lists: m outside
 * [1, 2048], k outside [1, m]); n_rows / nq < 0; n_rows * k or nq * m above 2^31 - 1; a filter that srx_search_filtered
 * would refuse (NULL or misaligned bits, n_filters < 1); with rows to do, a NULL out_doc, out_key, out_extra (lists: also
 * cand_doc, cand_score, out_score) or workspace, or a workspace that is not 8-byte aligned.
 *
 * Not covered: several sort keys; ordering by a function of score and value (boosts, decay); SET64 columns; a sharded index
 * (columns and rows are shard-local); k above 1024 in one call (page with the cursor); lists above 2048.
 */
#ifndef SPARSE_RX_ORDER_H
#define SPARSE_RX_ORDER_H

#include "sparse_rx_fields.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SRX_ORDER_ASC = 0, SRX_ORDER_DESC = 1 };
enum { SRX_ORDER_NULLS_LAST = 0, SRX_ORDER_NULLS_FIRST = 1, SRX_ORDER_NULLS_DROP = 2 };
#define SRX_ORDER_MAX_M 2048

int64_t srx_order_workspace_bytes(int64_t n_docs, int32_t n_rows, int32_t k); /* < 0: invalid arguments */

int srx_order_topk(int32_t device, const srx_field_col *col, int64_t n_docs, int64_t doc_base, int32_t order, int32_t nulls,
                   const srx_doc_filter *filter /* host struct or NULL */, int32_t n_rows, int32_t k,
                   const int32_t *after_doc /* device i32[n_rows] GLOBAL ids, or NULL */,
                   int32_t *out_doc /* i32[n_rows][k] GLOBAL ids */, int64_t *out_key /* i64[n_rows][k] */,
                   int32_t *out_extra /* i32[n_rows][3] = {count, valued, total} */, void *workspace, int64_t workspace_bytes,
                   void *stream);

int srx_order_lists(int32_t device, const srx_field_col *col, int64_t n_docs, int64_t doc_base, int32_t order, int32_t nulls,
                    const int32_t *cand_doc /* i32[nq][m] GLOBAL ids */, const float *cand_score /* f32[nq][m] */,
                    const int32_t *cand_count /* i32[nq] or NULL */, int32_t nq, int32_t m, int32_t k,
                    int32_t *out_doc /* i32[nq][k] */, float *out_score /* f32[nq][k] */, int64_t *out_key /* i64[nq][k] */,
                    int32_t *out_pos /* i32[nq][k] or NULL */, int32_t *out_extra /* i32[nq][3] = {count, valued, live} */,
                    void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_ORDER_H */
