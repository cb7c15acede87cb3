/* sparse_rx_ltr.h -- learned reranking: the scores of a ranked list replaced (or moved) by a tree-ensemble model over the
 * features the device already holds, and the list cut to its new top k, on the device.
 *
 * Fifteenth header of libsparse_rx.so (same library, same conventions as sparse_rx.h: extern "C", device pointers, negative
 * return codes, the message of the last failure from the error-text call of sparse_rx.h).
 *
 * Why: boost/sparse_rx_boost.h moves a score by curves the caller wrote by hand.  What production stacks put on this slot is a
 * LEARNED model (the Elasticsearch and Solr learning-to-rank plugins, Vespa's GBDT rank phase): a LambdaMART or gradient-boosting
 * forest over the retrieval score, the rank, metadata columns and features the caller computed.  The reference has no such
 * step: nothing here replaces reference code.
 *
 * A tree ensemble needs no transcendental function: its floating-point work is compares and ONE ordered fp32 sum, so the
 * contract is pinned bit for bit (tests/ltr_ref.py restates it).  Per-tree learning rates and a forest's averaging are folded
 * into the leaf values on the host: the node table is the contract.
 *
 * ---- the contract -----------------------------------------------------------------------------------------------------
 *
 * Columns      `cols` is a HOST array of 0 <= n_cols <= SRX_LTR_MAX_COLS = 8 descriptors of sparse_rx_fields.h, type
 *              SRX_FIELD_I32, SRX_FIELD_I64 or SRX_FIELD_F32: a device array of n_docs values, naturally aligned, and
 *              optionally ONE filter row `valid` (16-byte aligned; NULL = every doc has a value).  Row i belongs to the doc
 *              with the global id doc_base + i.  n_cols == 0 (cols is then not looked at) is legal when no feature names a
 *              column.
 * Features     `features` is a HOST array of 1 <= n_features <= SRX_LTR_MAX_FEATURES = 32 srx_ltr_feature {kind, index}.
 *              Feature f of the live candidate at position c of query q, with the local doc d, is
 *                SRX_LTR_F_SCORE   the candidate's raw score (index is not looked at);
 *                SRX_LTR_F_RANK    (float)c (index is not looked at);
 *                SRX_LTR_F_COLUMN  cols[index][d] converted to fp32, round to nearest even (what NumPy's
 *                                  .astype(float32) gives for int32 and int64); a cleared `valid` bit gives a NaN, and an
 *                                  F32 NaN stays one: "missing";
 *                SRX_LTR_F_EXTRA   extra[q][c][index] of the caller's DEVICE plane f32[nq][m][n_extra], 0 <= n_extra <=
 *                                  SRX_LTR_MAX_EXTRA = 32; a NaN means missing.
 * Model        a DEVICE array `nodes` of n_nodes srx_ltr_node (16 bytes each, 16-byte aligned) and a DEVICE array tree_ptr
 *              i32[n_trees + 1]; 1 <= n_trees <= SRX_LTR_MAX_TREES = 4096, 1 <= n_nodes <= SRX_LTR_MAX_NODES = 2^22.  The
 *              scalars `base` (fp32), `cmp` (SRX_LTR_LE: x <= value goes left; SRX_LTR_LT: x < value goes left) and `mode`.
 *              A node with feature < 0 is a LEAF and `value` its output.  Otherwise the low 16 bits of `feature` are the
 *              feature index, bit 30 (SRX_LTR_MISSING_LEFT) says "a missing value goes left", `value` is the threshold and
 *              `left` / `right` are node indices RELATIVE to the tree's first node.
 * Walk         of tree t over the nodes [b, e) = [tree_ptr[t], tree_ptr[t + 1]):
 *                1. not 0 <= b < e <= n_nodes (a range outside the table, or an empty one): the contribution is +0;
 *                2. start at i = b;
 *                3. node i is a leaf: the contribution is its value;
 *                4. its feature index is >= n_features: the contribution is +0;
 *                5. otherwise x is that feature.  The step goes LEFT if x is a NaN and bit 30 is set, or if the plain IEEE
 *                   compare (x <= value, x < value) holds; RIGHT otherwise.  So a NaN threshold sends every value right,
 *                   a NaN x without bit 30 goes right, and -0 equals +0;
 *                6. j = b + child, in 64 bits.  Not i < j < e: the contribution is +0.  Otherwise continue at 3 with i = j.
 *              Node indices increase strictly along a walk, so every walk ends, and a model with ARBITRARY contents causes
 *              no read outside `nodes` and `tree_ptr`.
 * New score    acc = base, then acc = acc + contribution_t for t = 0, 1, .., n_trees - 1 IN THAT ORDER, every add its own
 *              fp32 operation.  SRX_LTR_REPLACE: acc;  SRX_LTR_SUM: s + acc, s the raw score.  A NaN new score is stored
 *              as 0x7FC00000.
 * Candidates   cand_doc i32[nq][m] GLOBAL doc ids, cand_score f32[nq][m] RAW scores, cand_count i32[nq] or NULL, in any
 *              order.  1 <= m <= SRX_LTR_MAX_M = 2048, 1 <= k <= m.
 * Live         a candidate c of query q is LIVE iff
 *                - c < min(max(count[q], 0), m)   (a NULL count means m), and
 *                - its doc id minus doc_base, computed in 64 bits, is in [0, n_docs).
 * Selection    (srx_ltr_topk) the first k of all live positions by (new score descending, doc id ascending).  Scores compare
 *              by their order-mapped bits: +0 ranks ahead of -0, every NaN ranks after -inf (NaNs tie; the doc id decides).
 *              The result does not depend on the launch geometry.
 * Outputs      srx_ltr_topk: rows padded with -1 / +0.0f / -1; every word of every output row and every count is written.
 *                out_doc[q][t]    i32[nq][k]
 *                out_score[q][t]  f32[nq][k]  the new score
 *                out_count[q]     i32[nq]     min(k, live positions)
 *                out_pos[q][t]    i32[nq][k]  (may be NULL) the position in the list given
 *              srx_ltr_score: out_score f32[nq][m], the new score of every live position, +0.0f at every dead one; every
 *              word is written.  The outputs must not overlap the inputs.
 * Execution    asynchronous on `stream`; allocates nothing, needs no workspace, uses no global atomics; ONE launch.
 *              nq == 0 returns SRX_OK without a launch.  Everything given is only read.
 * Precondition, NOT checked: no doc id twice among the candidates of one query (srx_ltr_topk).
 *
 * Refused with SRX_ERR_INVALID before anything touches a device: n_cols outside 0 .. 8, a NULL cols with n_cols > 0; a column
 * with NULL data, data misaligned for its type (I32 / F32: 4 bytes, I64: 8), a type other than I32 / I64 / F32 (SET64: a label
 * set is no number), a valid row that is not 16-byte aligned; n_docs outside [1, 2^31 - 2] or a negative doc_base; a NULL
 * features, n_features outside 1 .. 32, n_extra outside 0 .. 32, a feature of an unknown kind, a COLUMN index outside
 * [0, n_cols), an EXTRA index outside [0, n_extra); n_trees outside 1 .. 4096, n_nodes outside 1 .. 2^22; a cmp or mode
 * outside its enum; m outside 1 .. 2048, k outside 1 .. m; nq < 0 or nq * m > 2^31 - 1; with nq > 0 a NULL cand_doc,
 * cand_score, out_doc, out_score or out_count (srx_ltr_score: out_score), a NULL nodes or tree_ptr, nodes not 16-byte
 * aligned, an EXTRA feature with a NULL extra.
 *
 * Not covered: SET64 columns and categorical splits; multi-output models; lists deeper than 2048; a sharded index (columns
 * are shard-local); training.
 */
#ifndef SPARSE_RX_LTR_H
#define SPARSE_RX_LTR_H

#include "sparse_rx_fields.h"

#ifdef __cplusplus
extern "C" {
#endif

enum { SRX_LTR_F_SCORE = 0, SRX_LTR_F_RANK = 1, SRX_LTR_F_COLUMN = 2, SRX_LTR_F_EXTRA = 3 }; /* srx_ltr_feature.kind */
enum { SRX_LTR_LE = 0, SRX_LTR_LT = 1 };                                                     /* cmp */
enum { SRX_LTR_REPLACE = 0, SRX_LTR_SUM = 1 };                                               /* mode */
#define SRX_LTR_MISSING_LEFT 1073741824 /* bit 30 of srx_ltr_node.feature */
#define SRX_LTR_MAX_M 2048
#define SRX_LTR_MAX_COLS 8
#define SRX_LTR_MAX_FEATURES 32
#define SRX_LTR_MAX_EXTRA 32
#define SRX_LTR_MAX_TREES 4096
#define SRX_LTR_MAX_NODES 4194304

typedef struct srx_ltr_feature { /* HOST array element, 8 bytes */
    int32_t kind;  /* SRX_LTR_F_* */
    int32_t index; /* COLUMN: into cols; EXTRA: into the plane's last axis */
} srx_ltr_feature;

typedef struct srx_ltr_node { /* DEVICE array element, 16 bytes */
    int32_t feature; /* < 0: a leaf; else low 16 bits = feature index, bit 30 = missing goes left */
    float value;     /* a leaf's output, else the threshold */
    int32_t left;    /* relative to the tree's first node */
    int32_t right;
} srx_ltr_node;

int srx_ltr_topk(int32_t device,
                 const srx_field_col *cols, int32_t n_cols, /* HOST array of sparse_rx_fields.h: I32 / I64 / F32 columns */
                 int64_t n_docs, int64_t doc_base,
                 const srx_ltr_feature *features, int32_t n_features, /* HOST */
                 const float *extra /* device f32[nq][m][n_extra], may be NULL when no feature is EXTRA */, int32_t n_extra,
                 const srx_ltr_node *nodes, int32_t n_nodes, const int32_t *tree_ptr, int32_t n_trees, /* device */
                 float base, int32_t cmp, int32_t mode,
                 const int32_t *cand_doc, const float *cand_score, const int32_t *cand_count /* may be NULL */,
                 int32_t nq, int32_t m, int32_t k,
                 int32_t *out_doc, float *out_score, int32_t *out_count, int32_t *out_pos /* may be NULL */,
                 void *stream);

int srx_ltr_score(int32_t device,
                  const srx_field_col *cols, int32_t n_cols,
                  int64_t n_docs, int64_t doc_base,
                  const srx_ltr_feature *features, int32_t n_features,
                  const float *extra, int32_t n_extra,
                  const srx_ltr_node *nodes, int32_t n_nodes, const int32_t *tree_ptr, int32_t n_trees,
                  float base, int32_t cmp, int32_t mode,
                  const int32_t *cand_doc, const float *cand_score, const int32_t *cand_count /* may be NULL */,
                  int32_t nq, int32_t m,
                  float *out_score /* f32[nq][m] */,
                  void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SPARSE_RX_LTR_H */
