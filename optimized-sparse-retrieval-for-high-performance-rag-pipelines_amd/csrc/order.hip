// order.hip -- order by a field (order/sparse_rx_order.h): the first k docs of a filter row, or of a result list, by the value
// one resident metadata column holds for them.
//
// Replaces nothing in the reference project: it has no field ordering.
//
// The RANK.  What the header's order compares is folded into 96 bits that compare as unsigned numbers, hi (64) then lo (32):
//     hi = class << 63 | u >> 1        lo = (u & 1) << 31 | tie
// u is the value mapped to an unsigned 64-bit number that ascends as the value does (integers: the sign bit flipped; F32: -0
// made +0, then the usual bit trick -- negative floats complemented, the others get the top bit), complemented under DESC; a
// doc without a value has u = 0.  class puts the valueless docs behind the valued ones (NULLS_LAST, NULLS_DROP) or in front
// (NULLS_FIRST).  tie is the local doc id (below 2^31) for rows and the position for lists.  1 + 64 + 31 bits: nothing is lost,
// the smaller rank precedes, and two docs never share a rank.  (~0, ~0) is no doc's rank: it pads the sorts and bounds the cuts.
// out_key is not decoded from the rank: it is read again from the column (k loads per row), so an F32 -0 stays -0.
//
// Row form, launch one: the scan.  Grid (segments, rows).  A workgroup walks one segment of one row in chunks of 8192 docs: every
// thread stages one row word and one validity word in LDS, then for 32 steps thread t looks at doc chunk + 256 step + t, so a
// wave's gathers of the column are 64 consecutive values.  A step without a set bit in a wave's 64 docs costs that wave two LDS
// reads; a chunk without a set bit costs its load.  A doc of the set whose rank lies behind the cursor's and in front of the
// THRESHOLD is appended to a list of CAP ranks in LDS (2048 for k <= 512: 26 KB, six workgroups per CU; 4096 above: 50 KB,
// three).  A GROUP of steps (CAP / 2 docs: 4 or 8 steps) first issues all its gathers, then ranks and appends; the barrier
// that closes a group carries out whether the fill passed CAP / 2 (one answer for the workgroup), and if so the list is CUT: sorted (bitonic, the 96-bit compare), its k-th rank
// becomes the threshold, the rest is dropped.  The segment's first min(k, kept) ranks, sorted, and its {kept, total} go to the
// workspace.
//
// The cut is a sort, not the radix selection of srx_common.h: radix_kth takes keys of 31 bits with 0 as "no key", so a 96-bit
// rank would be four chained selections over remapped digits; one sort routine serves the cut, the merge's ranking and the list
// form, and it runs once per CAP / 2 - k ranks that beat the threshold, not per doc.
//
// Launch two: the merge.  One workgroup per row streams the segments' lists through the same append / cut and ranks the result.
//
// List form.  One workgroup per list: the rank of every live position (tie = the position: a stable sort), one sort of at most
// 2048 ranks, the first k are written.
//
// Integer work only, LDS atomics only (the list's fill): every workgroup owns the words it writes.
//
// The checks of the column, of n_docs / doc_base and of the lists, the validity bit and the column load are field_common.h's.
#include "field_common.h"
#include "order/sparse_rx_order.h"

namespace {

constexpr int OD_CAP_SMALL = 2048;            // ranks of a workgroup's list for k <= 512 (24 KB of LDS) ...
constexpr int OD_CAP = 4096;                  // ... and above (48 KB).  Half of it is the BATCH: the most appends between two looks at the fill
constexpr int OD_CHUNK = THREADS * 32;        // docs staged per round: one row word per thread
constexpr int64_t OD_MIN_SEG = 32768;         // a segment is max(OD_MIN_SEG, 64 k) docs, rounded up to whole chunks
constexpr int OD_MAX_ROWS_Y = 65535;          // grid.y; more rows than that are looped over
constexpr int OD_LIST_CAP = SRX_ORDER_MAX_M;

struct OrderArgs {
    const void *data;            // the column
    const uint32_t *valid;       // one filter row, or null
    int type, order, nulls;
    int64_t n_docs, doc_base, words;
    int k;
    // row form
    const uint32_t *base_bits;   // null = every doc
    const int32_t *base_q;       // null = base row 0
    const int32_t *after_doc;    // [n_rows] or null
    int n_rows, segments;
    int64_t seg_docs;
    uint64_t *ws_hi;             // [n_rows][segments][k]
    uint32_t *ws_lo;             // [n_rows][segments][k]
    int32_t *ws_cnt;             // [n_rows][segments][2] = {kept, total}
    int32_t *out_doc;            // [rows][k]
    int64_t *out_key;            // [rows][k]
    int32_t *out_extra;          // [rows][3]
    // list form
    const int32_t *cand_doc;     // [nq][m]
    const float *cand_score;     // [nq][m]
    const int32_t *cand_count;   // [nq] or null
    float *out_score;            // [nq][k]
    int32_t *out_pos;            // [nq][k] or null
    int m;
};

struct Rank {
    uint64_t hi;
    uint32_t lo;
};
__device__ __forceinline__ bool od_less(const Rank &a, const Rank &b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }

template <int CAP>
struct OrderShared {
    uint64_t hi[CAP];
    uint32_t lo[CAP];
    unsigned count, total, valued;
    Rank thr;
};

// ---- the value of a doc (tests/order_ref.py restates these)
__device__ __forceinline__ bool od_valid_bit(const uint32_t *valid, uint32_t d) {
    return valid == nullptr || srx_field_valid_bit(valid, d);
}
// the value as out_key holds it; d < n_docs
__device__ __forceinline__ int64_t od_raw(const OrderArgs &a, uint32_t d) {
    return srx_field_load(a.data, a.type == SRX_FIELD_I64, a.type == SRX_FIELD_F32, d);
}
// u of the header comment; false: a NaN, no value
__device__ __forceinline__ bool od_map(const OrderArgs &a, int64_t raw, uint64_t &u) {
    if (a.type == SRX_FIELD_F32) {
        uint32_t b = (uint32_t)raw;
        if ((b & 0x7FFFFFFFu) > 0x7F800000u) return false;
        if ((b << 1) == 0u) b = 0u;  // -0 == +0
        u = (b >> 31) ? ~b : (b | 0x80000000u);
    } else {
        u = (uint64_t)raw ^ (1ull << 63);
    }
    if (a.order == SRX_ORDER_DESC) u = ~u;
    return true;
}
// the rank of a doc whose validity bit is `on` and whose column entry is `raw` (read only when on); *has: the doc has a value
__device__ __forceinline__ Rank od_rank(const OrderArgs &a, bool on, int64_t raw, uint32_t tie, bool *has) {
    uint64_t u = 0;
    bool h = on;
    if (on) h = od_map(a, raw, u);
    if (!h) u = 0;
    *has = h;
    const uint64_t cls = h == (a.nulls == SRX_ORDER_NULLS_FIRST) ? 1ull : 0ull;
    return {(cls << 63) | (u >> 1), ((uint32_t)(u & 1ull) << 31) | tie};
}
__device__ __forceinline__ bool od_rank_has(const OrderArgs &a, uint64_t hi) { return ((hi >> 63) != 0ull) == (a.nulls == SRX_ORDER_NULLS_FIRST); }

// ---- the list in LDS
// Ascending bitonic sort of the first cnt ranks (cnt <= CAP, the same value in every thread, the ranks visible); the places up to
// the next power of two are filled with (~0, ~0).  Ends with a barrier.
template <int CAP>
__device__ void od_sort(OrderShared<CAP> &S, unsigned cnt) {
    const unsigned tid = threadIdx.x;
    unsigned n = 1;
    while (n < cnt) n <<= 1;  // <= CAP: CAP is a power of two
    for (unsigned i = cnt + tid; i < n; i += THREADS) S.hi[i] = ~0ull, S.lo[i] = ~0u;
    __syncthreads();
    for (unsigned size = 2; size <= n; size <<= 1) {
        for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
            for (unsigned i = tid; i < (n >> 1); i += THREADS) {
                const unsigned pos = 2 * i - (i & (stride - 1));  // pos + stride < n
                const Rank x = {S.hi[pos], S.lo[pos]}, y = {S.hi[pos + stride], S.lo[pos + stride]};
                const bool asc = (pos & size) == 0;
                if (asc ? od_less(y, x) : od_less(x, y)) {
                    S.hi[pos] = y.hi, S.lo[pos] = y.lo;
                    S.hi[pos + stride] = x.hi, S.lo[pos + stride] = x.lo;
                }
            }
            __syncthreads();
        }
    }
}

// Cut the list to its k first ranks; the k-th becomes the threshold.  Every thread of the workgroup calls it or none does, with no
// append in flight: the callers take the decision out of a barrier (od_cut_due).  Ends with a barrier.
template <int CAP>
__device__ void od_cut(OrderShared<CAP> &S, int k) {
    const unsigned cnt = S.count;
    od_sort(S, cnt);
    if (threadIdx.x == 0 && cnt > (unsigned)k) {
        S.count = (unsigned)k;
        S.thr = {S.hi[k - 1], S.lo[k - 1]};
    }
    __syncthreads();
}
// The barrier that closes a batch of appends, and whether a cut is due before the next one: the same answer in every thread.
// A thread looks at the fill after its own appends; appends are atomic adds on one word, so the thread that made the batch's last
// one sees them all, and the barrier ORs the looks.  (A look at the top of the next batch is NOT uniform: a wave that arrives
// late would see what faster waves have already appended to that batch, and enter the cut's barriers alone.)
template <int CAP>
__device__ __forceinline__ bool od_cut_due(OrderShared<CAP> &S) { return __syncthreads_or(S.count > (unsigned)(CAP / 2)) != 0; }
// one rank more: the batch rule keeps the fill within CAP
template <int CAP>
__device__ __forceinline__ void od_push(OrderShared<CAP> &S, const Rank &r) {
    const unsigned p = atomicAdd(&S.count, 1u);
    S.hi[p] = r.hi, S.lo[p] = r.lo;
}

// the cursor of row r: false = none; otherwise only ranks behind *low stay ((~0, ~0): none does)
__device__ __forceinline__ bool od_cursor(const OrderArgs &a, int r, Rank *low) {
    const int c = a.after_doc != nullptr ? cload_i32(a.after_doc + r) : -1;
    if (c == -1) return false;
    *low = {~0ull, ~0u};
    const int64_t local = (int64_t)c - a.doc_base;
    if (local >= 0 && local < a.n_docs) {
        bool has;
        const bool on = od_valid_bit(a.valid, (uint32_t)local);
        const Rank rk = od_rank(a, on, on ? od_raw(a, (uint32_t)local) : 0, (uint32_t)local, &has);
        if (has || a.nulls != SRX_ORDER_NULLS_DROP) *low = rk;
    }
    return true;
}

template <int CAP>
__global__ __launch_bounds__(THREADS) void srx_order_scan_kernel(OrderArgs a) {
    constexpr int BATCH = CAP / 2, STEPS = BATCH / THREADS, GROUPS = 32 / STEPS;  // a chunk is 32 steps of 256 docs
    __shared__ OrderShared<CAP> S;
    __shared__ uint32_t s_row[THREADS], s_ok[THREADS];  // a chunk's staged row and validity words
    const int tid = threadIdx.x, lane = tid & 63;
    const int seg = blockIdx.x;
    const int64_t d_begin = (int64_t)seg * a.seg_docs;  // < n_docs; a multiple of OD_CHUNK
    const int64_t d_end = d_begin + a.seg_docs < a.n_docs ? d_begin + a.seg_docs : a.n_docs;
    const bool drop = a.nulls == SRX_ORDER_NULLS_DROP;
    for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
        if (tid == 0) {
            S.count = 0u, S.total = 0u;
            S.thr = {~0ull, ~0u};
        }
        Rank low = {0ull, 0u};
        const bool low_on = od_cursor(a, r, &low);
        const int br = srx_filter_base_row(a.base_bits, a.base_q, r);
        const uint32_t *brow = br >= 0 ? a.base_bits + (int64_t)br * a.words : nullptr;
        unsigned total = 0;  // wave-uniform
        bool cut_due = false;  // uniform: the list is empty
        __syncthreads();
        for (int64_t c0 = d_begin; c0 < d_end; c0 += OD_CHUNK) {
            const int64_t w = (c0 >> 5) + tid;
            uint32_t bits = srx_filter_word_docs(a.n_docs, w * 32), okw = ~0u;  // 0 from n_docs on: a loaded word lies inside its row
            if (bits != 0u && brow != nullptr) bits &= (uint32_t)gload_i32((const int32_t *)brow + w);
            if (bits != 0u && a.valid != nullptr) okw = (uint32_t)gload_i32((const int32_t *)a.valid + w);
            s_row[tid] = bits, s_ok[tid] = okw;
            if (!__syncthreads_or(bits != 0u)) continue;  // nothing read the staged words: the next round may overwrite them
            for (int g = 0; g < GROUPS; ++g) {
                if (cut_due) od_cut(S, a.k);  // at most CAP / 2 ranks stay: room for a batch
                const Rank thr = S.thr;
                bool in[STEPS], on[STEPS];
                int64_t raw[STEPS];
#pragma unroll
                for (int s = 0; s < STEPS; ++s) {  // the group's gathers, all in flight together
                    const int i = (g * STEPS + s) * THREADS + tid;  // < OD_CHUNK
                    in[s] = (s_row[i >> 5] >> (i & 31)) & 1u;
                    on[s] = in[s] && ((s_ok[i >> 5] >> (i & 31)) & 1u);
                    raw[s] = 0;
                    if (on[s]) raw[s] = od_raw(a, (uint32_t)(c0 + i));  // a set bit lies below n_docs: the load is inside the column
                }
#pragma unroll
                for (int s = 0; s < STEPS; ++s) {
                    const uint64_t mask = __ballot(in[s]);
                    if (mask == 0ull) continue;
                    total += (unsigned)__popcll(mask);
                    if (in[s]) {
                        const uint32_t d = (uint32_t)(c0 + (g * STEPS + s) * THREADS + tid);
                        bool has;
                        const Rank rk = od_rank(a, on[s], raw[s], d, &has);
                        if ((has || !drop) && (!low_on || od_less(low, rk)) && od_less(rk, thr)) od_push(S, rk);
                    }
                }
                cut_due = od_cut_due(S);  // also: the staged words are read, the next chunk may overwrite them
            }
        }
        if (lane == 0 && total != 0u) atomicAdd(&S.total, total);
        __syncthreads();
        const unsigned cnt = S.count;
        od_sort(S, cnt);
        const unsigned kept = cnt < (unsigned)a.k ? cnt : (unsigned)a.k;
        const int64_t slot = (int64_t)r * a.segments + seg;
        for (unsigned i = tid; i < kept; i += THREADS) {
            a.ws_hi[slot * a.k + i] = S.hi[i];
            a.ws_lo[slot * a.k + i] = S.lo[i];
        }
        if (tid == 0) {
            a.ws_cnt[slot * 2] = (int32_t)kept;
            a.ws_cnt[slot * 2 + 1] = (int32_t)S.total;
        }
        __syncthreads();  // before the next row resets the list
    }
}

template <int CAP>
__global__ __launch_bounds__(THREADS) void srx_order_merge_kernel(OrderArgs a) {
    constexpr int BATCH = CAP / 2;
    __shared__ OrderShared<CAP> S;
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.x;
    const int k = a.k;
    if (tid == 0) {
        S.count = 0u, S.total = 0u, S.valued = 0u;
        S.thr = {~0ull, ~0u};
    }
    __syncthreads();
    const int32_t *cnt_row = a.ws_cnt + r * a.segments * 2;
    unsigned total = 0;
    for (int s = tid; s < a.segments; s += THREADS) total += (unsigned)gload_i32(cnt_row + 2 * s + 1);
    if (total != 0u) atomicAdd(&S.total, total);
    const int64_t n_in = (int64_t)a.segments * k;  // <= 2^26
    const uint64_t *in_hi = a.ws_hi + r * n_in;
    const uint32_t *in_lo = a.ws_lo + r * n_in;
    bool cut_due = false;  // uniform: the list is empty
    for (int64_t i0 = 0; i0 < n_in; i0 += BATCH) {
        if (cut_due) od_cut(S, k);
        const Rank thr = S.thr;
        for (int j = 0; j < BATCH / THREADS; ++j) {
            const int64_t i = i0 + j * THREADS + tid;
            if (i < n_in) {
                const int s = (int)(i / k), e = (int)(i - (int64_t)s * k);
                if (e < gload_i32(cnt_row + 2 * s)) {  // a rank the scan wrote
                    const Rank rk = {in_hi[i], in_lo[i]};
                    if (od_less(rk, thr)) od_push(S, rk);
                }
            }
        }
        cut_due = od_cut_due(S);
    }
    const unsigned cnt = S.count;
    od_sort(S, cnt);
    const unsigned kept = cnt < (unsigned)k ? cnt : (unsigned)k;
    for (unsigned i = tid; i < (unsigned)k; i += THREADS) {
        int32_t doc = -1;
        int64_t key = 0;
        if (i < kept) {
            const uint32_t d = S.lo[i] & 0x7FFFFFFFu;  // a doc of the set: below n_docs
            doc = (int32_t)(a.doc_base + d);
            if (od_rank_has(a, S.hi[i])) {
                key = od_raw(a, d);
                atomicAdd(&S.valued, 1u);
            }
        }
        a.out_doc[r * k + i] = doc;
        a.out_key[r * k + i] = key;
    }
    __syncthreads();
    if (tid == 0) {
        a.out_extra[r * 3] = (int32_t)kept;
        a.out_extra[r * 3 + 1] = (int32_t)S.valued;
        a.out_extra[r * 3 + 2] = (int32_t)S.total;
    }
}

__global__ __launch_bounds__(THREADS) void srx_order_lists_kernel(OrderArgs a) {
    __shared__ OrderShared<OD_LIST_CAP> S;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int m = a.m, k = a.k;
    int n = a.cand_count != nullptr ? cload_i32(a.cand_count + q) : m;  // the live prefix of the list
    n = n < 0 ? 0 : n > m ? m : n;
    const int32_t *row_doc = a.cand_doc + q * m;
    if (tid == 0) S.count = 0u, S.total = 0u, S.valued = 0u;
    __syncthreads();
    for (int i = tid; i < n; i += THREADS) {  // i < n <= m <= OD_LIST_CAP: inside the row and the list
        Rank rk = {~0ull, ~0u};
        const int64_t local = (int64_t)gload_i32(row_doc + i) - a.doc_base;
        if (local >= 0 && local < a.n_docs) {
            atomicAdd(&S.total, 1u);
            bool has;
            const bool on = od_valid_bit(a.valid, (uint32_t)local);
            const Rank x = od_rank(a, on, on ? od_raw(a, (uint32_t)local) : 0, (uint32_t)i, &has);
            if (has || a.nulls != SRX_ORDER_NULLS_DROP) {
                rk = x;
                atomicAdd(&S.count, 1u);
            }
        }
        S.hi[i] = rk.hi, S.lo[i] = rk.lo;
    }
    __syncthreads();
    od_sort(S, (unsigned)n);
    const unsigned sorted = S.count;  // the places behind them hold (~0, ~0)
    const unsigned kept = sorted < (unsigned)k ? sorted : (unsigned)k;
    const int32_t *row_bits = (const int32_t *)(a.cand_score + q * m);
    for (unsigned i = tid; i < (unsigned)k; i += THREADS) {
        int32_t doc = -1, pos = -1, bits = 0;
        int64_t key = 0;
        if (i < kept) {
            pos = (int32_t)(S.lo[i] & 0x7FFFFFFFu);  // a live position: below n, its doc inside the index
            doc = gload_i32(row_doc + pos);
            bits = gload_i32(row_bits + pos);
            if (od_rank_has(a, S.hi[i])) {
                key = od_raw(a, (uint32_t)((int64_t)doc - a.doc_base));
                atomicAdd(&S.valued, 1u);
            }
        }
        a.out_doc[q * k + i] = doc;
        ((int32_t *)a.out_score)[q * k + i] = bits;
        a.out_key[q * k + i] = key;
        if (a.out_pos != nullptr) a.out_pos[q * k + i] = pos;
    }
    __syncthreads();
    if (tid == 0) {
        a.out_extra[q * 3] = (int32_t)kept;
        a.out_extra[q * 3 + 1] = (int32_t)S.valued;
        a.out_extra[q * 3 + 2] = (int32_t)S.total;
    }
}

int64_t od_seg_docs(int k) {
    const int64_t want = 64ll * k > OD_MIN_SEG ? 64ll * k : OD_MIN_SEG;
    return (want + OD_CHUNK - 1) / OD_CHUNK * OD_CHUNK;
}

// what both entry points check of the column, the index and the order
int check_order(const char *who, const srx_field_col *col, int64_t n_docs, int64_t doc_base, int order, int nulls) {
    if (!col) return fail(SRX_ERR_INVALID, "%s: null col", who);
    const int rc = srx_check_field_cols(who, col, 1, SRX_FIELD_TYPES_NUMBER, "a SET64 column has no order");
    if (rc != SRX_OK) return rc;
    if (order != SRX_ORDER_ASC && order != SRX_ORDER_DESC) return fail(SRX_ERR_INVALID, "%s: unknown order", who);
    if (nulls != SRX_ORDER_NULLS_LAST && nulls != SRX_ORDER_NULLS_FIRST && nulls != SRX_ORDER_NULLS_DROP) return fail(SRX_ERR_INVALID, "%s: unknown nulls mode", who);
    return srx_check_field_docs(who, n_docs, doc_base, true);  // out_doc holds doc_base + d as an int32
}

void fill_col(OrderArgs &a, const srx_field_col *col, int64_t n_docs, int64_t doc_base, int order, int nulls, int k) {
    memset(&a, 0, sizeof(a));
    a.data = col->data, a.valid = col->valid, a.type = col->type;
    a.order = order, a.nulls = nulls, a.k = k;
    a.n_docs = n_docs, a.doc_base = doc_base, a.words = srx_filter_row_words(n_docs);
}

}  // namespace

SRX_API int64_t srx_order_workspace_bytes(int64_t n_docs, int32_t n_rows, int32_t k) {
    if (n_docs < 1 || n_docs > SRX_FILTER_MAX_DOCS || n_rows < 0 || k < 1 || k > SRX_MAX_K || (int64_t)n_rows * k > 0x7FFFFFFFll) return -1;
    const int64_t seg_docs = od_seg_docs(k), segments = (n_docs + seg_docs - 1) / seg_docs;
    return (int64_t)n_rows * segments * (12ll * k + 8);
}

SRX_API int srx_order_topk(int32_t device, const srx_field_col *col, int64_t n_docs, int64_t doc_base, int32_t order, int32_t nulls,
                           const srx_doc_filter *filter, int32_t n_rows, int32_t k, const int32_t *after_doc, int32_t *out_doc,
                           int64_t *out_key, int32_t *out_extra, void *workspace, int64_t workspace_bytes, void *stream_v) {
    const char *who = "srx_order_topk";
    const int rc = check_order(who, col, n_docs, doc_base, order, nulls);
    if (rc != SRX_OK) return rc;
    if (k < 1 || k > SRX_MAX_K) return fail(SRX_ERR_INVALID, "%s: k must be in [1, 1024]", who);
    if (n_rows < 0) return fail(SRX_ERR_INVALID, "%s: n_rows < 0", who);
    if ((int64_t)n_rows * k > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: n_rows * k must not exceed 2^31 - 1", who);
    if (filter) {
        const int frc = srx_check_filter(who, filter);
        if (frc != SRX_OK) return frc;
    }
    if (n_rows == 0) return SRX_OK;
    if (!out_doc || !out_key || !out_extra) return fail(SRX_ERR_INVALID, "%s: null out_doc / out_key / out_extra", who);
    if (!workspace) return fail(SRX_ERR_INVALID, "%s: null workspace", who);
    if ((uintptr_t)workspace & 7) return fail(SRX_ERR_INVALID, "%s: the workspace must be 8-byte aligned", who);
    if (workspace_bytes < srx_order_workspace_bytes(n_docs, n_rows, k)) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    OrderArgs a;
    fill_col(a, col, n_docs, doc_base, order, nulls, k);
    a.base_bits = filter ? filter->bits : nullptr;
    a.base_q = filter ? filter->q_filter : nullptr;
    a.after_doc = after_doc;
    a.n_rows = n_rows;
    a.seg_docs = od_seg_docs(k);
    a.segments = (int)((n_docs + a.seg_docs - 1) / a.seg_docs);  // <= 2^16
    const int64_t ranks = (int64_t)n_rows * a.segments * k;
    a.ws_hi = (uint64_t *)workspace;
    a.ws_lo = (uint32_t *)(a.ws_hi + ranks);
    a.ws_cnt = (int32_t *)(a.ws_lo + ranks);
    a.out_doc = out_doc, a.out_key = out_key, a.out_extra = out_extra;
    const dim3 scan_grid((unsigned)a.segments, (unsigned)(n_rows < OD_MAX_ROWS_Y ? n_rows : OD_MAX_ROWS_Y));
    if (4 * k <= OD_CAP_SMALL) {  // a cut leaves k ranks: at most a quarter of the list, so a cut is not due again after every batch
        hipLaunchKernelGGL(srx_order_scan_kernel<OD_CAP_SMALL>, scan_grid, dim3(THREADS), 0, stream, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(srx_order_merge_kernel<OD_CAP_SMALL>, dim3((unsigned)n_rows), dim3(THREADS), 0, stream, a);
    } else {
        hipLaunchKernelGGL(srx_order_scan_kernel<OD_CAP>, scan_grid, dim3(THREADS), 0, stream, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(srx_order_merge_kernel<OD_CAP>, dim3((unsigned)n_rows), dim3(THREADS), 0, stream, a);
    }
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int srx_order_lists(int32_t device, const srx_field_col *col, int64_t n_docs, int64_t doc_base, int32_t order, int32_t nulls,
                            const int32_t *cand_doc, const float *cand_score, const int32_t *cand_count, int32_t nq, int32_t m, int32_t k,
                            int32_t *out_doc, float *out_score, int64_t *out_key, int32_t *out_pos, int32_t *out_extra, void *stream_v) {
    const char *who = "srx_order_lists";
    int rc = check_order(who, col, n_docs, doc_base, order, nulls);
    if (rc == SRX_OK) rc = srx_check_list_shape(who, m, SRX_ORDER_MAX_M, k);
    if (rc == SRX_OK) rc = srx_check_lists(who, nq, m, cand_doc, cand_score, out_doc && out_score && out_key && out_extra, "null out_doc / out_score / out_key / out_extra");
    if (rc != SRX_OK) return rc < 0 ? rc : SRX_OK;  // SRX_LISTS_EMPTY: nothing to do
    HIP_TRY(hipSetDevice(device));
    OrderArgs a;
    fill_col(a, col, n_docs, doc_base, order, nulls, k);
    a.cand_doc = cand_doc, a.cand_score = cand_score, a.cand_count = cand_count, a.m = m;
    a.out_doc = out_doc, a.out_score = out_score, a.out_key = out_key, a.out_pos = out_pos, a.out_extra = out_extra;
    hipLaunchKernelGGL(srx_order_lists_kernel, dim3((unsigned)nq), dim3(THREADS), 0, (hipStream_t)stream_v, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
