// boost.hip -- field-value boosts (boost/sparse_rx_boost.h): the raw scores of a candidate list moved by up to eight curves over
// resident metadata columns, merged with a carry of final scores and cut to the first k by (score descending, doc ascending).
//
// Replaces nothing in the reference project: it has no score boosting.
//
// One workgroup per query, one launch per call, no workspace and no global atomics.  Three steps:
//
//   resolve  thread 0 turns every clause into what the factor stage needs -- the column's pointers and type, the curve's first
//            knot, (float)n_seg -- and leaves it in LDS; a clause that names no column or whose knots leave the table is marked
//            and treats every doc as one without a value (nothing of it is dereferenced).  The column is picked by a compare chain over the eight
//            descriptors of the kernel argument, not by an index: a runtime index would move the argument to scratch.
//   factor   thread t owns the positions t, t + 256, ..: the loads of the doc ids and scores are contiguous, the column values
//            and the two knots are gathers.  Per clause the value's offset from the origin goes through the clamped lerp of
//            the header, every operation rounded on its own (the unit is built with -ffp-contract=off, and says so again
//            below).  The clause records are LDS broadcasts.  A live position becomes the 64-bit KEY
//                ~map(score) << 32 | doc        map(b) = b >> 31 ? ~b : b | 0x80000000, a NaN -> 0
//            so that the ascending order of the keys is the header's order, two positions never share a key (no doc twice) and
//            ~0 is no position's key: it marks the dead ones and pads the sort.
//   cut      one ascending bitonic sort of (key, position) over the next power of two of m + kc (at most 2048: 16 KB of keys and
//            4 KB of 16-bit positions in LDS), then the first k are written.  A candidate's score is decoded from its key (the
//            map is a bijection off the NaNs, which are stored as 0x7FC00000); a carry entry's bits are read again from the
//            carry, so that a NaN payload survives.
//
// A sort, not a selection: k goes up to m + kc and the output is ranked, so a selection would still sort its k survivors; the
// sort network is the one order.hip uses for its lists, restated here for a 64-bit key (that unit is neither edited nor included).
//
// The checks of the columns and of n_docs / doc_base and the column helpers are field_common.h's; the carry's checks are woven into the list's, which stay here.
#include "field_common.h"
#include "boost/sparse_rx_boost.h"

#pragma clang fp contract(off)

namespace {

constexpr int BS_MAX_M = SRX_BOOST_MAX_M;
constexpr uint64_t BS_DEAD = ~0ull;

struct BoostCol {
    const void *data;
    const uint32_t *valid;
    int type;
};

struct BoostArgs {
    BoostCol cols[SRX_BOOST_MAX_COLS];
    const srx_boost_clause *clauses;
    const float *knots;
    const int32_t *cand_doc;     // [nq][m]
    const float *cand_score;     // [nq][m]
    const int32_t *cand_count;   // [nq] or null
    const int32_t *carry_doc;    // [nq][kc] or null
    const float *carry_score;    // [nq][kc] or null
    const int32_t *carry_count;  // [nq] or null
    int32_t *out_doc;            // [nq][k]
    float *out_score;            // [nq][k]
    int32_t *out_count;          // [nq]
    int32_t *out_pos;            // [nq][k] or null
    int64_t n_docs, doc_base;
    int n_cols, n_clauses, n_knots, score_mode, boost_mode, m, kc, k;
};

// a clause as the factor stage reads it; type < 0: the clause is unusable, every doc is without a value (f = missing)
struct BoostCurve {
    const void *data;
    const uint32_t *valid;
    const float *y;
    int64_t origin;
    float inv_step, weight, missing, n_seg_f;
    int type, abs, n_seg, pad;
};

__device__ __forceinline__ uint32_t bs_map(uint32_t b) {
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0u;  // a NaN: behind -inf (whose map is 0x007FFFFF)
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
// the bits a key's map stands for; 0 is the NaNs'
__device__ __forceinline__ uint32_t bs_unmap(uint32_t u) { return u == 0u ? 0x7FC00000u : (u >> 31) ? (u ^ 0x80000000u) : ~u; }

// g_c of the header for the local doc d < n_docs
__device__ __forceinline__ float bs_factor(const BoostCurve &c, uint32_t d) {
    if (c.type < 0) return c.weight * c.missing;
    if (c.valid != nullptr && !srx_field_valid_bit(c.valid, d)) return c.weight * c.missing;
    float x;
    if (c.type == SRX_FIELD_F32) {
        const uint32_t b = (uint32_t)srx_field_i32(c.data, d);
        if ((b & 0x7FFFFFFFu) > 0x7F800000u) return c.weight * c.missing;
        x = __uint_as_float(b) - __uint_as_float((uint32_t)c.origin);
    } else {
        // written out: through srx_field_load the kernel compiles to other code
        const int64_t v = c.type == SRX_FIELD_I64 ? srx_field_i64(c.data, d) : (int64_t)srx_field_i32(c.data, d);
        x = (float)((double)v - (double)c.origin);
    }
    if (c.abs) x = fabsf(x);
    const float t = x * c.inv_step;
    const SRX_GLOBAL float *y = (const SRX_GLOBAL float *)c.y;
    float f;
    if (!(t > 0.0f)) {
        f = y[0];
    } else if (t >= c.n_seg_f) {
        f = y[c.n_seg];
    } else {
        const int i = (int)t;  // 0 <= i < n_seg: i + 1 is a knot of the clause
        const float fr = t - (float)i;
        const float y0 = y[i], y1 = y[i + 1];
        const float dy = y1 - y0;
        const float step = fr * dy;
        f = y0 + step;
    }
    return c.weight * f;
}

__global__ __launch_bounds__(THREADS) void srx_boost_kernel(BoostArgs a) {
    __shared__ uint64_t s_key[BS_MAX_M];
    __shared__ uint16_t s_pos[BS_MAX_M];
    __shared__ BoostCurve s_curve[SRX_BOOST_MAX_CLAUSES];
    __shared__ unsigned s_live;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int m = a.m, kc = a.kc, k = a.k, total = kc + m;  // total <= BS_MAX_M

    // ---- resolve
    if (tid == 0) {
        s_live = 0u;
        for (int c = 0; c < a.n_clauses; ++c) {  // n_clauses <= 8: inside s_curve
            const srx_boost_clause cl = a.clauses[c];
            BoostCurve r;
            r.data = nullptr, r.valid = nullptr, r.y = nullptr, r.type = -1, r.pad = 0;
#pragma unroll
            for (int j = 0; j < SRX_BOOST_MAX_COLS; ++j)
                if (j == cl.col && j < a.n_cols) r.data = a.cols[j].data, r.valid = a.cols[j].valid, r.type = a.cols[j].type;
            if (cl.n_seg < 1 || cl.knot0 < 0 || (int64_t)cl.knot0 + cl.n_seg >= (int64_t)a.n_knots) r.type = -1;
            if (r.type >= 0) r.y = a.knots + cl.knot0;
            r.origin = cl.origin, r.inv_step = cl.inv_step, r.weight = cl.weight, r.missing = cl.missing;
            r.n_seg = cl.n_seg, r.n_seg_f = (float)cl.n_seg, r.abs = cl.flags & SRX_BOOST_ABS;
            s_curve[c] = r;
        }
    }
    __syncthreads();

    // ---- factor
    int n_carry = 0;
    if (kc > 0) {
        n_carry = a.carry_count != nullptr ? cload_i32(a.carry_count + q) : kc;
        n_carry = n_carry < 0 ? 0 : n_carry > kc ? kc : n_carry;
    }
    int n_cand = a.cand_count != nullptr ? cload_i32(a.cand_count + q) : m;
    n_cand = n_cand < 0 ? 0 : n_cand > m ? m : n_cand;
    unsigned n2 = 1;
    while (n2 < (unsigned)total) n2 <<= 1;  // <= BS_MAX_M: a power of two
    unsigned live = 0;
    for (unsigned i = tid; i < n2; i += THREADS) {
        uint64_t key = BS_DEAD;
        if ((int)i < kc) {
            if ((int)i < n_carry) {  // i < kc: inside the carry row
                const int doc = gload_i32(a.carry_doc + q * kc + i);
                const int64_t local = (int64_t)doc - a.doc_base;
                if (local >= 0 && local < a.n_docs) {
                    const uint32_t b = (uint32_t)gload_i32((const int32_t *)a.carry_score + q * kc + i);
                    key = ((uint64_t)(~bs_map(b)) << 32) | (uint32_t)doc;
                }
            }
        } else if ((int)i - kc < n_cand) {  // i - kc < m: inside the candidate row
            const int c0 = (int)i - kc;
            const int doc = gload_i32(a.cand_doc + q * m + c0);
            const int64_t local = (int64_t)doc - a.doc_base;
            if (local >= 0 && local < a.n_docs) {
                const float s = __int_as_float(gload_i32((const int32_t *)a.cand_score + q * m + c0));
                float F = bs_factor(s_curve[0], (uint32_t)local);
                for (int c = 1; c < a.n_clauses; ++c) {
                    const float g = bs_factor(s_curve[c], (uint32_t)local);
                    if (a.score_mode == SRX_BOOST_SCORE_MULTIPLY) F = F * g;
                    else if (a.score_mode == SRX_BOOST_SCORE_SUM) F = F + g;
                    else if (a.score_mode == SRX_BOOST_SCORE_MAX) F = g > F ? g : F;
                    else F = g < F ? g : F;
                }
                const float ns = a.boost_mode == SRX_BOOST_MULTIPLY ? s * F : a.boost_mode == SRX_BOOST_SUM ? s + F : F;
                key = ((uint64_t)(~bs_map(__float_as_uint(ns))) << 32) | (uint32_t)doc;  // doc >= doc_base >= 0: below 2^31, so key != BS_DEAD
            }
        }
        live += key != BS_DEAD;
        s_key[i] = key;  // i < n2 <= BS_MAX_M
        s_pos[i] = (uint16_t)i;
    }
    if (live != 0u) atomicAdd(&s_live, live);
    __syncthreads();

    // ---- cut: ascending bitonic sort of the n2 (key, position) pairs
    for (unsigned size = 2; size <= n2; size <<= 1) {
        for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
            for (unsigned i = tid; i < (n2 >> 1); i += THREADS) {
                const unsigned pos = 2 * i - (i & (stride - 1));  // pos + stride < n2
                const uint64_t x = s_key[pos], y = s_key[pos + stride];
                const bool asc = (pos & size) == 0;
                if (asc ? y < x : x < y) {
                    const uint16_t px = s_pos[pos], py = s_pos[pos + stride];
                    s_key[pos] = y, s_key[pos + stride] = x;
                    s_pos[pos] = py, s_pos[pos + stride] = px;
                }
            }
            __syncthreads();
        }
    }

    const unsigned all = s_live;
    const unsigned cnt = all < (unsigned)k ? all : (unsigned)k;  // the first `all` places hold the live positions
    const int64_t o = q * k;
    for (unsigned t = tid; t < (unsigned)k; t += THREADS) {  // k <= total <= n2
        int32_t doc = -1, pos = -1;
        uint32_t bits = 0u;
        if (t < cnt) {
            const uint64_t key = s_key[t];
            pos = (int32_t)s_pos[t];  // a live position: inside its row
            doc = (int32_t)(uint32_t)key;
            bits = pos < kc ? (uint32_t)gload_i32((const int32_t *)a.carry_score + q * kc + pos) : bs_unmap(~(uint32_t)(key >> 32));
        }
        a.out_doc[o + t] = doc;
        ((uint32_t *)a.out_score)[o + t] = bits;
        if (a.out_pos != nullptr) a.out_pos[o + t] = pos;
    }
    if (tid == 0) a.out_count[q] = (int32_t)cnt;
}

}  // namespace

SRX_API int srx_boost_topk(int32_t device, const srx_field_col *cols, int32_t n_cols, int64_t n_docs, int64_t doc_base,
                           const srx_boost_clause *clauses, int32_t n_clauses, const float *knots, int32_t n_knots, int32_t score_mode,
                           int32_t boost_mode, const int32_t *cand_doc, const float *cand_score, const int32_t *cand_count,
                           const int32_t *carry_doc, const float *carry_score, const int32_t *carry_count, int32_t nq, int32_t m, int32_t kc,
                           int32_t k, int32_t *out_doc, float *out_score, int32_t *out_count, int32_t *out_pos, void *stream_v) {
    const char *who = "srx_boost_topk";
    static_assert(sizeof(srx_boost_clause) == 40, "srx_boost_clause is 40 bytes");
    if (!cols) return fail(SRX_ERR_INVALID, "%s: null cols", who);
    if (n_cols < 1 || n_cols > SRX_BOOST_MAX_COLS) return fail(SRX_ERR_INVALID, "%s: n_cols must be in [1, 8]", who);
    int rc = srx_check_field_cols(who, cols, n_cols, SRX_FIELD_TYPES_NUMBER, "a SET64 column is no number to boost by");
    if (rc == SRX_OK) rc = srx_check_field_docs(who, n_docs, doc_base, false);
    if (rc != SRX_OK) return rc;
    if (n_clauses < 1 || n_clauses > SRX_BOOST_MAX_CLAUSES) return fail(SRX_ERR_INVALID, "%s: n_clauses must be in [1, 8]", who);
    if (n_knots < 2 || n_knots > SRX_BOOST_MAX_KNOTS) return fail(SRX_ERR_INVALID, "%s: n_knots must be in [2, 2^24]", who);
    if (score_mode < SRX_BOOST_SCORE_MULTIPLY || score_mode > SRX_BOOST_SCORE_MIN) return fail(SRX_ERR_INVALID, "%s: unknown score_mode", who);
    if (boost_mode < SRX_BOOST_MULTIPLY || boost_mode > SRX_BOOST_REPLACE) return fail(SRX_ERR_INVALID, "%s: unknown boost_mode", who);
    if (m < 1) return fail(SRX_ERR_INVALID, "%s: m must be >= 1", who);
    if (kc < 0) return fail(SRX_ERR_INVALID, "%s: kc must be >= 0", who);
    if ((int64_t)m + kc > SRX_BOOST_MAX_M) return fail(SRX_ERR_INVALID, "%s: m + kc must not exceed 2048", who);
    if (k < 1 || k > m + kc) return fail(SRX_ERR_INVALID, "%s: k must be in [1, m + kc]", who);
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if ((int64_t)nq * (m + kc) > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: nq * (m + kc) must not exceed 2^31 - 1", who);
    if (kc == 0 && (carry_doc || carry_score || carry_count)) return fail(SRX_ERR_INVALID, "%s: a carry given with kc == 0", who);
    if (nq == 0) return SRX_OK;
    if (!clauses || !knots) return fail(SRX_ERR_INVALID, "%s: null clauses / knots", who);
    if (!cand_doc || !cand_score) return fail(SRX_ERR_INVALID, "%s: null cand_doc / cand_score", who);
    if (kc > 0 && (!carry_doc || !carry_score)) return fail(SRX_ERR_INVALID, "%s: kc > 0 needs carry_doc and carry_score", who);
    if (!out_doc || !out_score || !out_count) return fail(SRX_ERR_INVALID, "%s: null out_doc / out_score / out_count", who);
    HIP_TRY(hipSetDevice(device));
    BoostArgs a;
    memset(&a, 0, sizeof(a));
    for (int j = 0; j < n_cols; ++j) a.cols[j].data = cols[j].data, a.cols[j].valid = cols[j].valid, a.cols[j].type = cols[j].type;
    a.clauses = clauses, a.knots = knots;
    a.cand_doc = cand_doc, a.cand_score = cand_score, a.cand_count = cand_count;
    a.carry_doc = carry_doc, a.carry_score = carry_score, a.carry_count = carry_count;
    a.out_doc = out_doc, a.out_score = out_score, a.out_count = out_count, a.out_pos = out_pos;
    a.n_docs = n_docs, a.doc_base = doc_base;
    a.n_cols = n_cols, a.n_clauses = n_clauses, a.n_knots = n_knots, a.score_mode = score_mode, a.boost_mode = boost_mode;
    a.m = m, a.kc = kc, a.k = k;
    hipLaunchKernelGGL(srx_boost_kernel, dim3((unsigned)nq), dim3(THREADS), 0, (hipStream_t)stream_v, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
