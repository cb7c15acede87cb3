// ltr.hip -- learned reranking (ltr/sparse_rx_ltr.h): the raw scores of a candidate list replaced or moved by a tree ensemble
// over up to 32 features -- the score, the rank, resident metadata columns, a caller's plane -- and the list cut to the first k
// by (new score descending, doc ascending) (srx_ltr_topk), or every position's new score written out (srx_ltr_score).
//
// Replaces nothing in the reference project: it has no learned reranking.
//
// One workgroup per query, one launch per call, no workspace and no global atomics.  The list is taken in TILES of 256
// candidates, thread t owning candidate tile * 256 + t; a tile past the query's count is not looked at.  Per tile:
//
//   gather   the tile's features go to LDS feature-major, s_feat[f][t]: a lane's read of ANY feature sits in its own bank, so the
//            walk's LDS reads are conflict-free whatever node each lane stands on.  Doc ids and scores are contiguous loads, a
//            column value is a gather, an extra-plane entry a load at the stride of n_extra floats (the features of one candidate
//            share its cache lines).  The features' records are resolved once per workgroup (threads 0 .. n_features - 1) into
//            LDS: the column is picked by a compare chain over the eight descriptors of the kernel argument, the record from four
//            packed words, not by an index: a runtime index would move the argument to scratch.
//   walk     thread t walks ALL trees for its candidate, in tree order, and adds each contribution to its fp32 accumulator: the
//            order of the sum is the contract, so trees are not split across threads.  A step is one 16-byte node load (the
//            model is shared by every workgroup and stays in L2), one LDS read and a compare.  Steps 1, 4 and 6 of the header's
//            walk are the bounds checks: whatever the model holds, no node outside [b, e) within [0, n_nodes) is read, and no
//            feature row outside s_feat.
//
// Then (srx_ltr_topk) a live position becomes the 64-bit KEY
//                ~map(score) << 32 | doc        map(b) = b >> 31 ? ~b : b | 0x80000000, a NaN -> 0
// so that the ascending order of the keys is the header's order, two positions never share a key (no doc twice) and ~0 is no
// position's key: it marks the dead ones and pads the sort;
//
//   cut      one ascending bitonic sort of (key, position) over the next power of two of m (at most 2048: 16 KB of keys and 4 KB
//            of 16-bit positions in LDS), then the first k are written, the score decoded from its key (the map is a bijection
//            off the NaNs, which are stored as 0x7FC00000).
//
// The sort network is the one boost.hip uses, restated here (neither that unit nor order.hip is edited or included).  The model
// is not staged in LDS: see DESIGN 4.24.  The checks of the columns, of n_docs / doc_base and of the lists are field_common.h's.
#include "field_common.h"
#include "ltr/sparse_rx_ltr.h"

#pragma clang fp contract(off)

namespace {

constexpr int LT_MAX_M = SRX_LTR_MAX_M;
constexpr int LT_TILE = THREADS;
constexpr uint64_t LT_DEAD = ~0ull;
constexpr uint32_t LT_NAN = 0x7FC00000u;

struct LtrCol {
    const void *data;
    const uint32_t *valid;
    int type;
};

struct LtrArgs {
    LtrCol cols[SRX_LTR_MAX_COLS];
    uint64_t feat[4];            // feature f: byte f & 7 of word f >> 3 = kind | index << 2
    const float *extra;          // [nq][m][n_extra] or null
    const srx_ltr_node *nodes;   // [n_nodes]
    const int32_t *tree_ptr;     // [n_trees + 1]
    const int32_t *cand_doc;     // [nq][m]
    const float *cand_score;     // [nq][m]
    const int32_t *cand_count;   // [nq] or null
    int32_t *out_doc;            // [nq][k]       (topk)
    float *out_score;            // [nq][k]       (topk)   [nq][m] (score)
    int32_t *out_count;          // [nq]          (topk)
    int32_t *out_pos;            // [nq][k] or null
    int64_t n_docs, doc_base;
    float base;
    int n_cols, n_features, n_extra, n_nodes, n_trees, cmp, mode, m, k;
};

// a feature as the gather stage reads it
struct LtrFeat {
    const void *data;
    const uint32_t *valid;
    int kind, index, type, pad;
};

__device__ __forceinline__ uint32_t lt_map(uint32_t b) {
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0u;  // a NaN: behind -inf (whose map is 0x007FFFFF)
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ uint32_t lt_unmap(uint32_t u) { return u == 0u ? LT_NAN : (u >> 31) ? (u ^ 0x80000000u) : ~u; }

// the new score of the candidate whose features are column `tid` of s_feat
__device__ __forceinline__ float lt_walk(const LtrArgs &a, const float (*s_feat)[LT_TILE], int tid, float s) {
    float acc = a.base;
    for (int t = 0; t < a.n_trees; ++t) {
        const int b = cload_i32(a.tree_ptr + t), e = cload_i32(a.tree_ptr + t + 1);  // t + 1 <= n_trees: inside tree_ptr
        float contrib = 0.0f;
        if (b >= 0 && b < e && e <= a.n_nodes) {
            int i = b;
            for (;;) {  // b <= i < e <= n_nodes: inside nodes
                const srx_i4u nd = gload_i4((const int32_t *)a.nodes + 4 * (int64_t)i);
                if (nd.x < 0) {
                    contrib = __int_as_float(nd.y);
                    break;
                }
                const int fi = nd.x & 0xFFFF;
                if (fi >= a.n_features) break;
                const float x = s_feat[fi][tid];  // fi < n_features <= 32: a row of s_feat
                const float v = __int_as_float(nd.y);
                const bool left = x != x ? (nd.x & SRX_LTR_MISSING_LEFT) != 0 : a.cmp == SRX_LTR_LE ? x <= v : x < v;
                const int64_t j = (int64_t)b + (left ? nd.z : nd.w);
                if (!(j > (int64_t)i && j < (int64_t)e)) break;
                i = (int)j;
            }
        }
        acc = acc + contrib;
    }
    return a.mode == SRX_LTR_REPLACE ? acc : s + acc;
}

// what the cut keeps in LDS; the score instance keeps nothing
template <bool TOPK>
struct LtrCut {};
template <>
struct LtrCut<true> {
    uint64_t key[LT_MAX_M];
    uint16_t pos[LT_MAX_M];
    unsigned live;
};

template <bool TOPK>
__global__ __launch_bounds__(THREADS) void srx_ltr_kernel(LtrArgs a) {
    __shared__ float s_feat[SRX_LTR_MAX_FEATURES][LT_TILE];
    __shared__ LtrFeat s_ft[SRX_LTR_MAX_FEATURES];
    __shared__ LtrCut<TOPK> s_cut;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int m = a.m;

    // ---- resolve
    if constexpr (TOPK) {
        if (tid == 0) s_cut.live = 0u;
    }
    if (tid < a.n_features) {  // n_features <= 32: inside s_ft
        const uint64_t w = tid < 8 ? a.feat[0] : tid < 16 ? a.feat[1] : tid < 24 ? a.feat[2] : a.feat[3];
        const int rec = (int)(w >> ((tid & 7) * 8)) & 0xFF;
        LtrFeat r;
        r.data = nullptr, r.valid = nullptr, r.kind = rec & 3, r.index = rec >> 2, r.type = -1, r.pad = 0;
        if (r.kind == SRX_LTR_F_COLUMN) {
#pragma unroll
            for (int j = 0; j < SRX_LTR_MAX_COLS; ++j)
                if (j == r.index && j < a.n_cols) r.data = a.cols[j].data, r.valid = a.cols[j].valid, r.type = a.cols[j].type;
        }
        s_ft[tid] = r;
    }
    __syncthreads();

    int n_cand = a.cand_count != nullptr ? cload_i32(a.cand_count + q) : m;
    n_cand = n_cand < 0 ? 0 : n_cand > m ? m : n_cand;
    unsigned n2 = 1;
    while (n2 < (unsigned)m) n2 <<= 1;  // <= LT_MAX_M: a power of two
    [[maybe_unused]] unsigned live = 0;

    for (int c0 = 0; c0 < n_cand; c0 += LT_TILE) {
        const int c = c0 + tid;
        // ---- gather
        bool alive = false;
        int doc = -1;
        float s = 0.0f;
        if (c < n_cand) {  // c < m: inside the candidate row
            doc = gload_i32(a.cand_doc + q * m + c);
            const int64_t local = (int64_t)doc - a.doc_base;
            if (local >= 0 && local < a.n_docs) {
                alive = true;
                s = __int_as_float(gload_i32((const int32_t *)a.cand_score + q * m + c));
                const uint32_t d = (uint32_t)local;
                for (int f = 0; f < a.n_features; ++f) {
                    const int kind = s_ft[f].kind;
                    float x;
                    if (kind == SRX_LTR_F_SCORE) {
                        x = s;
                    } else if (kind == SRX_LTR_F_RANK) {
                        x = (float)c;
                    } else if (kind == SRX_LTR_F_EXTRA) {  // index < n_extra, extra not null: checked on the host
                        x = __int_as_float(gload_i32((const int32_t *)a.extra + (q * m + c) * a.n_extra + s_ft[f].index));
                    } else {
                        const void *data = s_ft[f].data;
                        const uint32_t *valid = s_ft[f].valid;
                        const int type = s_ft[f].type;
                        if (type < 0 || (valid != nullptr && !srx_field_valid_bit(valid, d))) x = __uint_as_float(LT_NAN);
                        else if (type == SRX_FIELD_F32) x = srx_field_f32(data, d);
                        else if (type == SRX_FIELD_I64) x = (float)srx_field_i64(data, d);
                        else x = (float)srx_field_i32(data, d);
                    }
                    s_feat[f][tid] = x;  // the lane's own column: no other lane reads it, so no barrier before the walk
                }
            }
        }
        // ---- walk
        if constexpr (TOPK) {
            uint64_t key = LT_DEAD;
            if (alive) {
                const float ns = lt_walk(a, s_feat, tid, s);
                key = ((uint64_t)(~lt_map(__float_as_uint(ns))) << 32) | (uint32_t)doc;  // doc >= doc_base >= 0: below 2^31, so key != LT_DEAD
                live += 1u;
            }
            if (c < (int)n2) s_cut.key[c] = key, s_cut.pos[c] = (uint16_t)c;  // c < n2 <= LT_MAX_M
        } else if (c < m) {
            uint32_t bits = 0u;
            if (alive) {
                bits = __float_as_uint(lt_walk(a, s_feat, tid, s));
                if ((bits & 0x7FFFFFFFu) > 0x7F800000u) bits = LT_NAN;
            }
            ((uint32_t *)a.out_score)[q * m + c] = bits;
        }
    }
    // the positions no tile covered: dead
    const unsigned done = (unsigned)((n_cand + LT_TILE - 1) / LT_TILE) * LT_TILE;
    if constexpr (!TOPK) {
        for (unsigned i = done + tid; i < (unsigned)m; i += THREADS) ((uint32_t *)a.out_score)[q * m + i] = 0u;
    } else {
        for (unsigned i = done + tid; i < n2; i += THREADS) s_cut.key[i] = LT_DEAD, s_cut.pos[i] = (uint16_t)i;  // i < n2 <= LT_MAX_M
        if (live != 0u) atomicAdd(&s_cut.live, live);
        __syncthreads();

        // ---- cut: ascending bitonic sort of the n2 (key, position) pairs
        for (unsigned size = 2; size <= n2; size <<= 1) {
            for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
                for (unsigned i = tid; i < (n2 >> 1); i += THREADS) {
                    const unsigned pos = 2 * i - (i & (stride - 1));  // pos + stride < n2
                    const uint64_t x = s_cut.key[pos], y = s_cut.key[pos + stride];
                    const bool asc = (pos & size) == 0;
                    if (asc ? y < x : x < y) {
                        const uint16_t px = s_cut.pos[pos], py = s_cut.pos[pos + stride];
                        s_cut.key[pos] = y, s_cut.key[pos + stride] = x;
                        s_cut.pos[pos] = py, s_cut.pos[pos + stride] = px;
                    }
                }
                __syncthreads();
            }
        }

        const int k = a.k;
        const unsigned all = s_cut.live;
        const unsigned cnt = all < (unsigned)k ? all : (unsigned)k;  // the first `all` places hold the live positions
        const int64_t o = q * k;
        for (unsigned t = tid; t < (unsigned)k; t += THREADS) {  // k <= m <= n2
            int32_t doc = -1, pos = -1;
            uint32_t bits = 0u;
            if (t < cnt) {
                const uint64_t key = s_cut.key[t];
                pos = (int32_t)s_cut.pos[t];
                doc = (int32_t)(uint32_t)key;
                bits = lt_unmap(~(uint32_t)(key >> 32));
            }
            a.out_doc[o + t] = doc;
            ((uint32_t *)a.out_score)[o + t] = bits;
            if (a.out_pos != nullptr) a.out_pos[o + t] = pos;
        }
        if (tid == 0) a.out_count[q] = (int32_t)cnt;
    }
}

// everything both entry points check and fill alike (`has_k`: srx_ltr_topk).  SRX_LISTS_EMPTY: nothing to do.
int ltr_prepare(const char *who, LtrArgs &a, const srx_field_col *cols, int32_t n_cols, int64_t n_docs, int64_t doc_base,
                const srx_ltr_feature *features, int32_t n_features, const float *extra, int32_t n_extra, const srx_ltr_node *nodes,
                int32_t n_nodes, const int32_t *tree_ptr, int32_t n_trees, float base, int32_t cmp, int32_t mode, const int32_t *cand_doc,
                const float *cand_score, const int32_t *cand_count, int32_t nq, int32_t m, bool has_k, int32_t k, bool have_outs, const char *null_outs) {
    static_assert(sizeof(srx_ltr_node) == 16 && sizeof(srx_ltr_feature) == 8, "srx_ltr_node is 16 bytes, srx_ltr_feature 8");
    if (n_cols < 0 || n_cols > SRX_LTR_MAX_COLS) return fail(SRX_ERR_INVALID, "%s: n_cols must be in [0, 8]", who);
    if (n_cols > 0 && !cols) return fail(SRX_ERR_INVALID, "%s: null cols", who);
    int rc = n_cols > 0 ? srx_check_field_cols(who, cols, n_cols, SRX_FIELD_TYPES_NUMBER, "a SET64 column is no number to rank by") : SRX_OK;
    if (rc == SRX_OK) rc = srx_check_field_docs(who, n_docs, doc_base, false);
    if (rc != SRX_OK) return rc;
    if (!features) return fail(SRX_ERR_INVALID, "%s: null features", who);
    if (n_features < 1 || n_features > SRX_LTR_MAX_FEATURES) return fail(SRX_ERR_INVALID, "%s: n_features must be in [1, 32]", who);
    if (n_extra < 0 || n_extra > SRX_LTR_MAX_EXTRA) return fail(SRX_ERR_INVALID, "%s: n_extra must be in [0, 32]", who);
    bool any_extra = false;
    memset(&a, 0, sizeof(a));
    for (int f = 0; f < n_features; ++f) {
        const int kind = features[f].kind, index = features[f].index;
        if (kind < SRX_LTR_F_SCORE || kind > SRX_LTR_F_EXTRA) return fail(SRX_ERR_INVALID, "%s: unknown feature kind", who);
        if (kind == SRX_LTR_F_COLUMN && (index < 0 || index >= n_cols)) return fail(SRX_ERR_INVALID, "%s: a COLUMN feature's index must be in [0, n_cols)", who);
        if (kind == SRX_LTR_F_EXTRA && (index < 0 || index >= n_extra)) return fail(SRX_ERR_INVALID, "%s: an EXTRA feature's index must be in [0, n_extra)", who);
        any_extra |= kind == SRX_LTR_F_EXTRA;
        const uint64_t rec = (uint64_t)kind | (kind >= SRX_LTR_F_COLUMN ? (uint64_t)index << 2 : 0u);  // index < 32: seven bits
        a.feat[f >> 3] |= rec << ((f & 7) * 8);
    }
    if (n_trees < 1 || n_trees > SRX_LTR_MAX_TREES) return fail(SRX_ERR_INVALID, "%s: n_trees must be in [1, 4096]", who);
    if (n_nodes < 1 || n_nodes > SRX_LTR_MAX_NODES) return fail(SRX_ERR_INVALID, "%s: n_nodes must be in [1, 2^22]", who);
    if (cmp < SRX_LTR_LE || cmp > SRX_LTR_LT) return fail(SRX_ERR_INVALID, "%s: unknown cmp", who);
    if (mode < SRX_LTR_REPLACE || mode > SRX_LTR_SUM) return fail(SRX_ERR_INVALID, "%s: unknown mode", who);
    rc = srx_check_list_shape(who, m, SRX_LTR_MAX_M, has_k ? k : 1);
    if (rc == SRX_OK) rc = srx_check_lists(who, nq, m, cand_doc, cand_score, have_outs, null_outs);
    if (rc != SRX_OK) return rc;
    if (!nodes || !tree_ptr) return fail(SRX_ERR_INVALID, "%s: null nodes / tree_ptr", who);
    if ((uintptr_t)nodes & 15u) return fail(SRX_ERR_INVALID, "%s: nodes must be 16-byte aligned", who);
    if (any_extra && !extra) return fail(SRX_ERR_INVALID, "%s: an EXTRA feature needs the extra plane", who);
    for (int j = 0; j < n_cols; ++j) a.cols[j].data = cols[j].data, a.cols[j].valid = cols[j].valid, a.cols[j].type = cols[j].type;
    a.extra = extra, a.nodes = nodes, a.tree_ptr = tree_ptr;
    a.cand_doc = cand_doc, a.cand_score = cand_score, a.cand_count = cand_count;
    a.n_docs = n_docs, a.doc_base = doc_base, a.base = base;
    a.n_cols = n_cols, a.n_features = n_features, a.n_extra = n_extra, a.n_nodes = n_nodes, a.n_trees = n_trees, a.cmp = cmp, a.mode = mode;
    a.m = m, a.k = has_k ? k : 0;
    return SRX_OK;
}

}  // namespace

SRX_API int srx_ltr_topk(int32_t device, const srx_field_col *cols, int32_t n_cols, int64_t n_docs, int64_t doc_base, const srx_ltr_feature *features,
                         int32_t n_features, const float *extra, int32_t n_extra, const srx_ltr_node *nodes, int32_t n_nodes, const int32_t *tree_ptr,
                         int32_t n_trees, float base, int32_t cmp, int32_t mode, const int32_t *cand_doc, const float *cand_score,
                         const int32_t *cand_count, int32_t nq, int32_t m, int32_t k, int32_t *out_doc, float *out_score, int32_t *out_count,
                         int32_t *out_pos, void *stream_v) {
    const char *who = "srx_ltr_topk";
    LtrArgs a;
    const int rc = ltr_prepare(who, a, cols, n_cols, n_docs, doc_base, features, n_features, extra, n_extra, nodes, n_nodes, tree_ptr, n_trees, base, cmp,
                               mode, cand_doc, cand_score, cand_count, nq, m, true, k, out_doc && out_score && out_count, "null out_doc / out_score / out_count");
    if (rc != SRX_OK) return rc == SRX_LISTS_EMPTY ? SRX_OK : rc;
    HIP_TRY(hipSetDevice(device));
    a.out_doc = out_doc, a.out_score = out_score, a.out_count = out_count, a.out_pos = out_pos;
    hipLaunchKernelGGL(srx_ltr_kernel<true>, dim3((unsigned)nq), dim3(THREADS), 0, (hipStream_t)stream_v, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int srx_ltr_score(int32_t device, const srx_field_col *cols, int32_t n_cols, int64_t n_docs, int64_t doc_base, const srx_ltr_feature *features,
                          int32_t n_features, const float *extra, int32_t n_extra, const srx_ltr_node *nodes, int32_t n_nodes, const int32_t *tree_ptr,
                          int32_t n_trees, float base, int32_t cmp, int32_t mode, const int32_t *cand_doc, const float *cand_score,
                          const int32_t *cand_count, int32_t nq, int32_t m, float *out_score, void *stream_v) {
    const char *who = "srx_ltr_score";
    LtrArgs a;
    const int rc = ltr_prepare(who, a, cols, n_cols, n_docs, doc_base, features, n_features, extra, n_extra, nodes, n_nodes, tree_ptr, n_trees, base, cmp,
                               mode, cand_doc, cand_score, cand_count, nq, m, false, 0, out_score != nullptr, "null out_score");
    if (rc != SRX_OK) return rc == SRX_LISTS_EMPTY ? SRX_OK : rc;
    HIP_TRY(hipSetDevice(device));
    a.out_score = out_score;
    hipLaunchKernelGGL(srx_ltr_kernel<false>, dim3((unsigned)nq), dim3(THREADS), 0, (hipStream_t)stream_v, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
