/* sparse_rx_feedback.h -- relevance feedback: a query and a ranked list of feedback docs -> an expanded weighted query, on the
 * device, in the CSR form srx_search takes.
 *
 * Twelfth header of libsparse_rx.so, the first under include/ext/ (same library, same conventions as sparse_rx.h: extern "C",
 * device pointers, negative return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: every other header narrows or reorders what the sparse search found; none changes what it looks for.  Pseudo-relevance
 * feedback does (RM3 for BM25, Rocchio for learned-sparse indexes, Lucene's more_like_this with a list of docs as the whole
 * query): the query is rebuilt from the terms of its own top docs.  The engine is term-major; this call reads a DOC-major
 * forward index the caller keeps resident (row d = the (term, value) pairs of local doc d, the most characteristic first) and
 * leaves the result on the device, so a first search, the expansion and the second search run without a copy back.  The
 * reference has no feedback: nothing here replaces reference code.
 *
 * ---- the contract -----------------------------------------------------------------------------------------------------
 * Every operation is rounded to fp32 on its own (no fused multiply-add), divisions are IEEE.  For query q:
 *
 * Used docs      positions r = 0, 1, ... below min(max(fb_count[q], 0), m, fb_docs) of row q of fb_doc / fb_score (a NULL
 *                fb_count means m).  Position r is USED when fb_doc - doc_base, computed in 64 bits, lies in [0, n_docs) and,
 *                under SRX_FB_BY_SCORE, 0 < fb_score < +inf (a NaN is not).  A doc listed twice is used twice.  The (doc,
 *                score, count) triple of any search can be passed as it is.  fb_score may be NULL under SRX_FB_UNIFORM.
 * Doc weights    BY_SCORE: S = the sum of the used scores in ascending r, starting from +0; a_r = score_r / S.
 *                UNIFORM: a_r = 1.0f / (float)n_used.
 * Contributions  the entries j < min(row length, row_cap) of the row of used doc r, in row order: p = value / doc_len[d]
 *                (SRX_FB_RM) or p = value (SRX_FB_RAW); c = a_r * p.  fb(t) = the sum of every c of term t in ascending r,
 *                starting from +0.
 * Selection      g(t) = term_gain[t], or 1 with a NULL term_gain.  Candidates: the terms with g(t) > 0 and fb(t) > 0.  Selected:
 *                the n_terms candidates with the largest fb(t) * g(t), ties to the smaller term id; all of them when there are
 *                fewer.  F = the sum of fb(t) over the selected terms in ascending term id, starting from +0.
 * Interpolation  Q = the sum of the query's weights in query order, starting from +0.  A term t of the query gets
 *                A = alpha * (qw(t) / Q) when Q > 0, any other term and every term when not Q > 0 gets A = +0.  A selected
 *                term gets B = beta * (fb(t) / F), any other B = +0.  w = A + B.
 * Output row     the union of the query's terms and the selected terms in ascending term id, each once, only the entries with
 *                w > 0.  out_ptr i32[nq + 1] is the exclusive prefix over the queries (out_ptr[0] = 0) and is written fully;
 *                out_term / out_weight are written below out_ptr[nq] and nowhere else.  *flag is written (0, or bit 0).
 * Over-long      a query of more than SRX_FEEDBACK_MAX_QTERMS terms is copied through unchanged (terms, weights, order) and
 *                bit 0 of *flag is set.
 *
 * Preconditions, NOT checked on the device: q_ptr starts at 0, ascends and ends at q_nnz; inside a query no term occurs twice
 * and 0 <= term < vocab (what srx_search requires; with a repeated term one of its weights counts, the row still lists it
 * once); row_ptr ascends from 0; inside a row of the forward index no term occurs twice.  A forward entry whose term lies
 * outside [0, vocab) is skipped; nothing is stored at or behind out_capacity whatever q_ptr holds.
 *
 * Execution      two launches, asynchronous on `stream`; allocates nothing.  One workgroup per query gathers at most
 *                fb_docs * row_cap <= 4096 (term, contribution) pairs into LDS, sorts them by (term, r) so that every sum
 *                runs in its defined order, selects, merges with the query and leaves a padded row in the workspace; the
 *                second launch scans the row lengths and compacts the rows.  Deterministic: a second call into the same
 *                buffers writes the same bytes.  nq == 0 returns SRX_OK without a launch.
 *
 * Refused with SRX_ERR_INVALID before anything touches a device: a NULL descriptor or params; n_docs outside [1, 2^31 - 2];
 * vocab outside [1, 2^26] (a (term, r) pair is a 32-bit sort key); a negative doc_base or doc_base + n_docs >= 2^31 - 1; fb_docs
 * outside [1, 32]; row_cap < 1; fb_docs * row_cap > 4096; n_terms outside [1, 128]; an unknown doc_weight or term_weight;
 * SRX_FB_RM without doc_len; alpha or beta negative or not finite, or both 0; nq < 0; m < 1 or nq * m > 2^31 - 1; q_nnz
 * outside [0, 2^31 - 1] or q_nnz + nq * n_terms > 2^31 - 1; out_capacity < q_nnz + nq * n_terms; with nq > 0 a NULL row_ptr,
 * term, value, q_ptr, fb_doc, out_ptr, out_term, out_weight or flag, a NULL q_term / q_weight with q_nnz > 0, a NULL fb_score
 * under BY_SCORE.  A NULL or too small workspace: SRX_ERR_NOMEM.
 *
 * Not covered: building the forward index (a sort of the CSR; the Python layer does it with torch); feedback from more than 32
 * docs or 4096 pairs per query; a sharded index (a forward index is shard-local, the feedback docs of a query are not).
 */
#ifndef SPARSE_RX_FEEDBACK_H
#define SPARSE_RX_FEEDBACK_H

#include "sparse_rx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SRX_FEEDBACK_MAX_DOCS    32    /* feedback docs used per query */
#define SRX_FEEDBACK_MAX_ENTRIES 4096  /* fb_docs * row_cap: (term, contribution) pairs a query gathers; 8 B each = 32 KB of the
                                          64 KB a statically sized LDS block may take, the rest is for the query and the output row */
#define SRX_FEEDBACK_MAX_TERMS   128   /* expansion terms selected per query */
#define SRX_FEEDBACK_MAX_QTERMS  128   /* terms of an input query */

enum { SRX_FB_BY_SCORE = 0, SRX_FB_UNIFORM = 1 }; /* srx_feedback_params.doc_weight */
enum { SRX_FB_RM = 0, SRX_FB_RAW = 1 };           /* srx_feedback_params.term_weight */

typedef struct srx_forward_desc { /* HOST struct of device pointers: the doc-major forward index */
    int32_t device, reserved;
    int64_t n_docs, vocab, doc_base;
    const int64_t *row_ptr;       /* i64[n_docs + 1] */
    const int32_t *term;          /* i32[nnz] */
    const float *value;           /* f32[nnz]: tf, or the learned weight */
    const float *doc_len;         /* f32[n_docs]; may be NULL (SRX_FB_RAW only) */
} srx_forward_desc;

typedef struct srx_feedback_params { /* HOST struct */
    int32_t fb_docs, row_cap, n_terms;
    int32_t doc_weight;  /* SRX_FB_BY_SCORE = 0, SRX_FB_UNIFORM = 1 */
    int32_t term_weight; /* SRX_FB_RM = 0: value / doc_len;  SRX_FB_RAW = 1: value */
    float alpha, beta;
} srx_feedback_params;

int64_t srx_feedback_workspace_bytes(int32_t nq);

int srx_feedback_expand(const srx_forward_desc *h_fwd, const srx_feedback_params *h_par, const float *term_gain /* f32[vocab] or NULL = 1 */,
                        const int32_t *q_ptr, const int32_t *q_term, const float *q_weight, int32_t nq, int64_t q_nnz /* host: q_ptr[nq] */,
                        const int32_t *fb_doc, const float *fb_score, const int32_t *fb_count /* or NULL */, int32_t m,
                        int32_t *out_ptr, int32_t *out_term, float *out_weight, int64_t out_capacity, int32_t *flag,
                        void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_FEEDBACK_H */
