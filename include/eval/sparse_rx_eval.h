/* sparse_rx_eval.h -- ranking evaluation: nDCG, AP, recall, precision, reciprocal rank and success of ranked lists against graded
 * relevance judgments, at several cutoffs per query, and their batch means, on the device.
 *
 * Sixteenth header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: every stage of the engine trades ranking quality for something, and nothing in it could say what was lost or won.  The
 * reference gets nDCG@k, MAP@k, Recall@k and P@k from BEIR's EvaluateRetrieval over pytrec_eval, on the host; nothing here
 * replaces reference code.  With the lists already on the device, model selection (a few thousand candidate rerankers over a large
 * development set) should bring back a handful of means per pass, not the lists.
 *
 * No metric needs a transcendental function once the gain and discount TABLES are sampled on the host (float64, rounded once to
 * fp32, as the knots of boost/sparse_rx_boost.h), so the contract is pinned bit for bit (tests/eval_ref.py restates it).  It uses
 * global doc ids and no shard-local column: it serves the merged lists of a sharded index too.
 *
 * ---- the contract -----------------------------------------------------------------------------------------------------
 *
 * Judgments    DEVICE arrays, a CSR over n_rows >= 0 judged queries, built once and kept resident:
 *                j_ptr    i64[n_rows + 1]  row r is the entries [j_ptr[r], j_ptr[r + 1]); a row that is not
 *                                          0 <= begin <= end <= nnz is an EMPTY row (nothing outside the arrays is read);
 *                j_doc    i32[nnz]         global doc ids, strictly ascending inside a row;
 *                j_grade  i32[nnz]         the grade of that doc;
 *                j_ideal  i32[nnz]         the same row's grades in descending order.
 *              A grade g is CLAMPED to [0, n_gain - 1]: a negative grade is judged but non-relevant.  A doc is RELEVANT iff its
 *              clamped grade is >= rel_level (rel_level >= 1).  R is the number of relevant docs of the row.
 * Tables       DEVICE arrays gain f32[n_gain], 1 <= n_gain <= SRX_EVAL_MAX_GAIN = 32, gain[0] = +0 ("linear": g, trec_eval's
 *              nDCG; "exp2": 2^g - 1), and discount f32[m] (1 / log2(r + 2) of position r).
 * Lists        cand_doc i32[nq][m] GLOBAL doc ids, cand_count i32[nq] or NULL, 1 <= m <= SRX_EVAL_MAX_M = 2048.  Position c is LIVE
 *              iff c < min(max(count[q], 0), m) (a NULL count means m).  Scores are no input: the list is taken in the order
 *              given.  A doc id that appears twice is counted at both positions (defined, not checked).
 * Rows         q_row i32[nq] or NULL (identity): the judgment row of list q.  A row outside [0, n_rows) -- -1 by convention -- means
 *              NOT JUDGED: every output of that query is 0 / +0 and the query is left out of the means.
 * Cutoffs      a HOST array ks i32[n_k], 1 <= n_k <= SRX_EVAL_MAX_K = 8, each >= 1, strictly ascending.  A cutoff may exceed m.
 *
 * Per query q and cutoff k let n = min(k, live positions).  For a position c < n: J_c is 1 iff cand_doc[q][c] is in the row; g_c
 * its clamped grade there, 0 if it is not; r_c is 1 iff J_c and g_c >= rel_level.
 *
 * Outputs      every word of every output is written; the outputs must not overlap the inputs.
 *                out_hits[q][ik]    i32[nq][n_k]  the sum of r_c over c < n
 *                out_judged[q][ik]  i32[nq][n_k]  the sum of J_c over c < n ("judged@k": the holes of the pool)
 *                out_rel[q]         i32[nq]       R
 *                out[q][ik][8]      f32[nq][n_k][8], every operation its own fp32 operation, no contraction:
 *                  SRX_EVAL_NDCG     0  DCG / IDCG, or +0 if IDCG == 0
 *                  SRX_EVAL_AP       1  (the sum over the relevant positions c < n, ascending, of
 *                                       (float)(hits through c) / (float)(c + 1)) / (float)R, or +0 if R == 0.  trec_eval's
 *                                       map_cut: the divisor is R, not min(R, k)
 *                  SRX_EVAL_RECALL   2  (float)hits / (float)R, or +0 if R == 0
 *                  SRX_EVAL_P        3  (float)hits / (float)k: the divisor is k even when the list is shorter
 *                  SRX_EVAL_RR       4  1 / (float)(c* + 1), c* the first relevant position < n; else +0
 *                  SRX_EVAL_SUCCESS  5  1.0 if hits > 0, else +0
 *                  SRX_EVAL_DCG      6  the sum over the positions c < n with gain[g_c] > 0, ascending, of gain[g_c] * discount[c],
 *                                       from +0
 *                  SRX_EVAL_IDCG     7  the same sum over i < min(k, row length, m) with gain[clamp(j_ideal[i])] > 0, times
 *                                       discount[i]
 *              The sums run over the contributing positions only, in ascending order, and are not re-associated.
 * Means        optional: out_mean f64[n_k][8] and out_n i32[1], both NULL or both given together with a workspace of
 *              srx_eval_workspace_bytes(nq, n_k) bytes, 8-byte aligned.  out_n is the number of EVALUATED queries (q_row valid).
 *              For each (cutoff, metric) the evaluated queries' values are converted to float64 and summed in CHUNKS of
 *              SRX_EVAL_MEAN_CHUNK = 1024 consecutive q, ascending; the chunk sums are summed ascending; the total is divided once
 *              by out_n; +0 if out_n is 0.  A query with R == 0 IS evaluated and contributes zeros (trec_eval's default over the
 *              queries in both files; its -c variant is host policy: pass an empty list for a judged query without results).
 * Execution    asynchronous on `stream`; allocates nothing, uses no global atomics; one launch for the per-query stage (one WAVE per
 *              query when m <= SRX_EVAL_WAVE_M = 256, a workgroup otherwise; a row of at most SRX_EVAL_LDS_ROW = 1024 judgments
 *              is staged in LDS, a longer one is searched in global memory) and two small ones for the means.  The result does not
 *              depend on the launch geometry.  nq == 0 returns SRX_OK without a launch and writes nothing.
 * Preconditions, NOT checked: j_doc strictly ascending inside a row (a doc of an unsorted row may be missed; nothing is read out
 *              of bounds); j_ideal the row's grades descending; gain[0] == +0 (an unjudged doc takes gain[0]).
 *
 * Refused with SRX_ERR_INVALID before anything touches a device: n_rows < 0 or nnz < 0; a NULL j_ptr, j_doc, j_grade or j_ideal
 * with n_rows > 0; n_gain outside 1 .. 32; a NULL gain or discount; rel_level < 1; m outside 1 .. 2048; n_k outside 1 .. 8, a
 * NULL ks, a cutoff < 1 or not strictly ascending; nq < 0 or nq * m > 2^31 - 1; with nq > 0 a NULL cand_doc, out, out_hits,
 * out_judged or out_rel; exactly one of out_mean / out_n NULL; means asked for with a workspace that is NULL, not 8-byte aligned
 * or smaller than srx_eval_workspace_bytes.
 *
 * Not covered: lists deeper than 2048; score ties (no re-sorting: the order given is the ranking); set-based measures over the
 * whole ranking (bpref, infAP); significance tests; training.
 */
#ifndef SPARSE_RX_EVAL_H
#define SPARSE_RX_EVAL_H

#include "sparse_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SRX_EVAL_NDCG = 0, SRX_EVAL_AP = 1, SRX_EVAL_RECALL = 2, SRX_EVAL_P = 3, SRX_EVAL_RR = 4, SRX_EVAL_SUCCESS = 5,
       SRX_EVAL_DCG = 6, SRX_EVAL_IDCG = 7 }; /* the last axis of out and out_mean */
#define SRX_EVAL_METRICS 8
#define SRX_EVAL_MAX_M 2048
#define SRX_EVAL_MAX_K 8
#define SRX_EVAL_MAX_GAIN 32
#define SRX_EVAL_WAVE_M 256
#define SRX_EVAL_LDS_ROW 1024
#define SRX_EVAL_MEAN_CHUNK 1024

/* bytes of the means' workspace; -1 for nq < 0 or n_k outside 1 .. 8 */
int64_t srx_eval_workspace_bytes(int32_t nq, int32_t n_k);

int srx_eval_lists(int32_t device,
                   const int64_t *j_ptr, const int32_t *j_doc, const int32_t *j_grade, const int32_t *j_ideal, /* device */
                   int32_t n_rows, int64_t nnz,
                   const float *gain, int32_t n_gain, const float *discount /* f32[m] */, int32_t rel_level,
                   const int32_t *cand_doc, const int32_t *cand_count /* may be NULL */, const int32_t *q_row /* may be NULL */,
                   int32_t nq, int32_t m,
                   const int32_t *ks /* HOST i32[n_k] */, int32_t n_k,
                   float *out /* f32[nq][n_k][8] */, int32_t *out_hits, int32_t *out_judged /* i32[nq][n_k] */, int32_t *out_rel /* i32[nq] */,
                   double *out_mean /* f64[n_k][8] or NULL */, int32_t *out_n /* i32[1] or NULL */,
                   void *workspace, int64_t workspace_bytes,
                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_EVAL_H */
