/* sparse_rx_boost.h -- field-value boosts: the scores of a ranked list moved by curves over metadata columns, and the list
 * cut to its new top k, on the device.
 *
 * Fourteenth header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: the columns of sparse_rx_fields.h can restrict a ranking (filters), count it (sparse_rx_facets.h), group it
 * (sparse_rx_collapse.h) and replace it (order/sparse_rx_order.h).  This header MIXES the two: "prefer recent passages",
 * "prefer answers with more votes", "down-weight docs far from this price" (Elasticsearch `function_score`, Qdrant's score
 * boosting formula, Vespa rank expressions over attributes).  The reference has no such step: nothing here replaces
 * reference code.
 *
 * A clause is ONE clamped, uniformly spaced, piecewise-linear curve over a signed or absolute offset from an origin.  Gauss,
 * exp and linear decay, log1p, sqrt and the identity are knot tables the host builds; the device contract holds no
 * transcendental function, so it is pinned bit for bit (tests/boost_ref.py restates it).
 *
 * It is a step over GIVEN lists.  The top k of the boosted COMPLETE ranking need a bound on what an unseen doc can reach; a
 * caller that wants them pages the search (the search-after entry point of sparse_rx.h) and passes "kept so far" as the
 * CARRY, whose scores are final, next to the next page of raw candidates.
 *
 * ---- the contract -----------------------------------------------------------------------------------------------------
 *
 * Columns      `cols` is a HOST array of 1 <= n_cols <= SRX_BOOST_MAX_COLS = 8 descriptors of sparse_rx_fields.h, type
 *              SRX_FIELD_I32, SRX_FIELD_I64 or SRX_FIELD_F32: a device array of n_docs values, naturally aligned, and
 *              optionally ONE filter row `valid` (16-byte aligned; NULL = every doc has a value).  Row i belongs to the doc
 *              with the global id doc_base + i.
 * Clauses      a DEVICE array of 1 <= n_clauses <= SRX_BOOST_MAX_CLAUSES = 8 srx_boost_clause (40 bytes each) and a DEVICE
 *              array knots f32[n_knots], 2 <= n_knots <= 2^24.  A clause names its column (0 <= col < n_cols) and its curve:
 *              the n_seg + 1 knots y = knots + knot0 (n_seg >= 1, knot0 >= 0, knot0 + n_seg < n_knots), inv_step (finite,
 *              > 0), weight, missing.  Their CONTENTS are the caller's responsibility; a clause that names no column or
 *              whose knots lie outside the table reads nothing out of bounds: every doc is without a value for it (f = missing).
 * Candidates   cand_doc i32[nq][m] GLOBAL doc ids, cand_score f32[nq][m] RAW scores, cand_count i32[nq] or NULL, in any
 *              order.  Carry: carry_doc i32[nq][kc], carry_score f32[nq][kc], carry_count i32[nq] or NULL, scores FINAL.
 *              1 <= m, 0 <= kc, m + kc <= SRX_BOOST_MAX_M = 2048, 1 <= k <= m + kc.  Position p of a query's list is carry
 *              entry p for p < kc and candidate p - kc otherwise.
 * Live         a candidate c (a carry entry c) of query q is LIVE iff
 *                - c < min(max(count[q], 0), m)   (kc for the carry; a NULL count means m / kc), and
 *                - its doc id minus doc_base, computed in 64 bits, is in [0, n_docs).
 * Factor       of clause c for a live candidate with the local doc d; every operation is rounded on its own (no fused
 *              multiply-add):
 *                1. the doc has NO value if its `valid` bit is 0, or if an F32 value is a NaN: f = missing.
 *                2. otherwise x = (float)((double)v - (double)origin) for I32 / I64, x = v - origin in fp32 for F32 (the
 *                   origin's float bits sit in the low 32 of `origin`);
 *                3. with SRX_BOOST_ABS, x = |x|;
 *                4. t = x * inv_step;  not (t > 0): f = y[0];  else t >= (float)n_seg: f = y[n_seg];  else i = (int)t,
 *                   fr = t - (float)i, f = y[i] + fr * (y[i+1] - y[i]);
 *                5. g_c = weight * f.
 *              F folds g_0 .. g_(n-1) left to right with score_mode: MULTIPLY a * b, SUM a + b, MAX (b > a ? b : a), MIN
 *              (b < a ? b : a) -- plain comparisons, the left operand stays on a tie (and when either is a NaN).
 * New score    boost_mode MULTIPLY: s * F;  SUM: s + F;  REPLACE: F.  A NaN new score is stored as 0x7FC00000.  Carry
 *              entries keep their score bits.
 * Selection    the first k of all live positions by (score descending, doc id ascending).  Scores compare by their
 *              order-mapped bits: +0 ranks ahead of -0, every NaN ranks after -inf (NaNs tie; the doc id decides).  The
 *              result does not depend on the launch geometry.
 * Outputs      rows padded with -1 / +0.0f / -1; every word of every output row and every count is written.
 *                out_doc[q][t]    i32[nq][k]
 *                out_score[q][t]  f32[nq][k]  the new score (a carry entry: the bits given)
 *                out_count[q]     i32[nq]     min(k, live positions)
 *                out_pos[q][t]    i32[nq][k]  (may be NULL) the position in carry ++ candidates
 *              The outputs must not overlap the inputs.
 * Execution    asynchronous on `stream`; allocates nothing, needs no workspace, uses no global atomics; ONE launch.
 *              nq == 0 returns SRX_OK without a launch.  Everything given is only read.
 * Precondition, NOT checked: no doc id twice in carry ++ candidates of one query.
 *
 * Refused with SRX_ERR_INVALID before anything touches a device: a NULL cols, n_cols outside 1 .. 8; a column with NULL
 * data, data misaligned for its type (I32 / F32: 4 bytes, I64: 8), a type other than I32 / I64 / F32 (SET64: a label set is
 * no number), a valid row that is not 16-byte aligned; n_docs outside [1, 2^31 - 2] or a negative doc_base; n_clauses
 * outside 1 .. 8, n_knots outside 2 .. 2^24; a score_mode or boost_mode outside its enum; m < 1, kc < 0, m + kc > 2048, k
 * outside 1 .. m + kc; nq < 0 or nq * (m + kc) > 2^31 - 1; with nq > 0 a NULL clauses, knots, cand_doc, cand_score, out_doc,
 * out_score or out_count; a carry_doc / carry_score / carry_count given with kc == 0, or kc > 0 with a NULL carry_doc or
 * carry_score.
 *
 * Not covered: SET64 columns; curves with unequal knot spacing (resample on the host); a product of two columns inside one
 * clause; a sharded index (columns are shard-local); lists deeper than 2048.
 */
#ifndef SPARSE_RX_BOOST_H
#define SPARSE_RX_BOOST_H

#include "sparse_rx_fields.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SRX_BOOST_SCORE_MULTIPLY = 0, SRX_BOOST_SCORE_SUM = 1, SRX_BOOST_SCORE_MAX = 2, SRX_BOOST_SCORE_MIN = 3 }; /* score_mode */
enum { SRX_BOOST_MULTIPLY = 0, SRX_BOOST_SUM = 1, SRX_BOOST_REPLACE = 2 };                                        /* boost_mode */
enum { SRX_BOOST_ABS = 1 };                                                                                       /* clause flags */
#define SRX_BOOST_MAX_M 2048
#define SRX_BOOST_MAX_CLAUSES 8
#define SRX_BOOST_MAX_COLS 8
#define SRX_BOOST_MAX_KNOTS 16777216

typedef struct srx_boost_clause { /* DEVICE array element, 40 bytes */
    int32_t col;      /* index into cols */
    int32_t flags;    /* bit 0: SRX_BOOST_ABS */
    int64_t origin;   /* F32 column: the float's bits in the low 32 */
    float inv_step;   /* finite, > 0 */
    float weight;
    float missing;
    int32_t knot0;    /* y = knots + knot0 */
    int32_t n_seg;    /* >= 1; knot0 + n_seg < n_knots */
    int32_t reserved; /* 0 */
} srx_boost_clause;

int srx_boost_topk(int32_t device,
                   const srx_field_col *cols, int32_t n_cols, /* HOST array of sparse_rx_fields.h: I32 / I64 / F32 columns */
                   int64_t n_docs, int64_t doc_base,
                   const srx_boost_clause *clauses, int32_t n_clauses, /* device */
                   const float *knots, int32_t n_knots,                /* device */
                   int32_t score_mode, int32_t boost_mode,
                   const int32_t *cand_doc, const float *cand_score, const int32_t *cand_count /* may be NULL */,
                   const int32_t *carry_doc, const float *carry_score, const int32_t *carry_count /* all NULL when kc == 0 */,
                   int32_t nq, int32_t m, int32_t kc, int32_t k,
                   int32_t *out_doc, float *out_score, int32_t *out_count, int32_t *out_pos /* may be NULL */,
                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_BOOST_H */
