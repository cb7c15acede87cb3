/* sparse_rx_facets.h -- facet counts: how the docs of a filter row, or of a result list, distribute over a field, on the device.
 *
 * Eleventh header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: sparse_rx_filter.h, sparse_rx_terms.h and sparse_rx_fields.h select a doc set, the searches rank it,
 * sparse_rx_collapse.h groups the ranking by a column.  What a search service prints next to its hits -- "wiki 812, arxiv 96,
 * forum 11", the hits per year, per price band (Elasticsearch `terms` / `range` / `histogram` aggregations, Solr facets, Vespa
 * grouping counts, Qdrant's facet API) -- needed the rows copied to the host and a second copy of the metadata walked there,
 * once per request.  The columns of sparse_rx_fields.h are resident, the rows have the layout of sparse_rx_filter.h and
 * every search returns (doc, count) lists: this header counts over them where they are.  The reference has no aggregation of
 * results: nothing here replaces reference code.
 *
 * ---- the contract -----------------------------------------------------------------------------------------------------
 *
 * Column       `col` is ONE descriptor of sparse_rx_fields.h in HOST memory: a device array of n_docs values of its type,
 *              naturally aligned (I32 / F32: 4 bytes, I64 / SET64: 8), and optionally ONE filter row `valid` (16-byte
 *              aligned; bit d set = local doc d has a value; NULL = every doc has one).
 * Doc set      srx_facet_counts, output row r: the base row, read exactly as srx_filter_from_fields reads its base -- a NULL
 *              `filter` means every doc; a NULL filter->q_filter means row 0; otherwise the row is q_filter[r] (i32[n_rows]),
 *              and -1 means every doc.  Only docs 0 <= d < n_docs count: bits at or above n_docs are never counted, even
 *              when they are set.
 *              srx_facet_counts_lists, list q: the LIVE positions of srx_collapse_topk, word for word -- position c is live
 *              iff c < min(max(cand_count[q], 0), m) (a NULL cand_count means m) and cand_doc[q][c] - doc_base, computed in
 *              64 bits, is in [0, n_docs).  Row i of the column belongs to the doc with the global id doc_base + i.  A doc id
 *              that occurs twice counts twice.  Scores are not taken.  m >= 1, nq * m <= 2^31 - 1.
 * Value        a counted doc HAS a value v when its `valid` bit is set, or when `valid` is NULL.
 * Bins         `bins` is a HOST struct.  The bin of a counted doc with the value v:
 *                SRX_FACET_CODES   I32 and I64 columns, widened to int64: bin v - origin when v >= origin and
 *                                  (uint64)(v - origin) < n_bins.  Nothing wraps: origin = INT64_MIN with v = INT64_MAX is
 *                                  "no bin".  1 <= n_bins <= 8192.  (Category codes, bools, years with an origin.)
 *                SRX_FACET_LABELS  SET64 columns: every bin i < n_bins with bit i of v set gets +1; a doc can count in several
 *                                  bins; bits at or above n_bins are ignored.  1 <= n_bins <= 64.
 *                SRX_FACET_EDGES   I32 / I64 / F32 columns: b = (number of j in [0, n_bins] with edges[j] <= v) - 1, and the doc
 *                                  counts in bin b when 0 <= b < n_bins -- bin b is [edges[b], edges[b + 1]).  `edges` is a
 *                                  DEVICE array i64[n_bins + 1], 8-byte aligned.  Integer columns compare as signed int64.  F32
 *                                  columns compare by IEEE on the float whose bits the entry holds in its low 32 bits: a NaN
 *                                  value is in no bin, -0 == +0.  1 <= n_bins <= 8192.
 *                                  Precondition, NOT checked on the device: the edges ascend (non-strictly) and none is NaN.
 *                                  Equal neighbours give an empty bin.  The kernel searches by bisection: edges that break
 *                                  the precondition give some bin or none, never a wild access.
 * Outputs      out_counts i32[rows][n_bins] and out_extra i32[rows][3] = {missing, other, total} per output row / list:
 *                missing  counted docs without a value;
 *                other    counted docs with a value that landed in no bin (LABELS: none of the low n_bins bits is set);
 *                total    counted docs.
 *              CODES and EDGES: sum(bins) + missing + other == total.  LABELS: sum(bins) is the sum of the popcounts of the
 *              masked values, and other + missing + (docs with at least one counted label) == total.
 *              Every word of both outputs is written; the call zeroes what it accumulates into, so a second call into the same
 *              buffers gives the same result.  The outputs must not overlap the inputs.
 * Execution    asynchronous on `stream`; allocates nothing, needs no workspace.  Integer atomics (LDS, and global for the row
 *              form): the result is exact and independent of order.  n_rows == 0 / nq == 0 returns SRX_OK without a launch.
 *              The column, the validity row, the edges, the filter rows and the candidate arrays are only read; they must not
 *              be written while a call that uses them is in flight.
 *
 * Refused with SRX_ERR_INVALID before anything touches a device: a NULL col; a NULL col->data, or data misaligned for its
 * type; an unknown column type; a valid row that is not 16-byte aligned; a NULL bins; a mode outside the enum; a mode that
 * does not fit the column's type (CODES: I32 / I64, LABELS: SET64, EDGES: I32 / I64 / F32); n_bins outside its range for the
 * mode; EDGES with NULL or 8-byte-misaligned edges; n_docs outside [1, 2^31 - 2]; (lists) a negative doc_base, or one with
 * doc_base + n_docs >= 2^31 - 1; n_rows / nq < 0; m < 1 or nq * m > 2^31 - 1; a filter that srx_search_filtered would refuse
 * (NULL or misaligned bits, n_filters < 1); with rows to do, a NULL cand_doc, out_counts or out_extra.
 *
 * Not covered: more than 8192 bins (a column with more distinct values is a key to collapse by, not a facet); sums, means,
 * minima or maxima per bin; nested facets (a facet per value of another field); selecting the top n bins on the device (the
 * host sorts at most 8192 numbers); a sharded index (columns and rows are shard-local).
 */
#ifndef SPARSE_RX_FACETS_H
#define SPARSE_RX_FACETS_H

#include "sparse_rx_fields.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SRX_FACET_CODES = 0, SRX_FACET_LABELS = 1, SRX_FACET_EDGES = 2 };
#define SRX_FACET_MAX_BINS 8192

typedef struct srx_facet_bins { /* HOST struct */
    int32_t mode, n_bins;       /* CODES / EDGES: 1 .. 8192; LABELS: 1 .. 64 */
    int64_t origin;             /* CODES only */
    const int64_t *edges;       /* EDGES only: device, i64[n_bins + 1]; F32 column: a float's bits in the low 32 */
} srx_facet_bins;

int srx_facet_counts(int32_t device, const srx_field_col *col, int64_t n_docs, const srx_facet_bins *bins,
                     const srx_doc_filter *filter /* host struct or NULL */, int32_t n_rows,
                     int32_t *out_counts /* i32[n_rows][n_bins] */, int32_t *out_extra /* i32[n_rows][3] */, void *stream);

int srx_facet_counts_lists(int32_t device, const srx_field_col *col, int64_t n_docs, int64_t doc_base, const srx_facet_bins *bins,
                           const int32_t *cand_doc /* i32[nq][m] GLOBAL ids */, const int32_t *cand_count /* i32[nq] or NULL */,
                           int32_t nq, int32_t m, int32_t *out_counts /* i32[nq][n_bins] */, int32_t *out_extra /* i32[nq][3] */,
                           void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_FACETS_H */
