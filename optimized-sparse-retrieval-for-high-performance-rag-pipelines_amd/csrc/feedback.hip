// feedback.hip -- relevance feedback (ext/sparse_rx_feedback.h): (query, ranked feedback docs) -> an expanded weighted query in
// the CSR form srx_search takes, from a resident doc-major forward index.
//
// Replaces nothing in the reference project: it has no feedback.
//
// Two launches per call, no global atomics but the one flag bit.
//
// srx_feedback_kernel: one workgroup of 256 threads per query.
//   docs     the first wave tests the <= 32 positions of the query's list; one thread adds the used scores in list order (the
//            sum is defined in that order) and lays the capped rows out back to back: at most fb_docs * row_cap <= 4096 pairs.
//   gather   wave w streams the rows r = w, w + 4, ...: consecutive lanes read consecutive (term, value) entries of one row,
//            and the pair (key = term << 5 | r, c = a_r * p) goes to LDS.  term < 2^26 and r < 32: the key has 31 bits.
//   sort     bitonic, ascending by key, over the next power of two of the pair count.  Equal terms then lie side by side in
//            ascending r, the order fb(t) is defined in: the first entry of a term walks its segment (<= 32 entries) serially.
//   select   a head whose term is a candidate carries the key bits(fb * g) + 1 (a product that underflows to +0 is still a
//            candidate).  More candidates than n_terms: the selection cut of srx_common.h (topk_cut over radix_kth -- the k-th
//            largest key, then the smallest term ids among its ties) with the heads' keys in registers, 16 per thread.
//   merge    the selected (term, fb) pairs and the query's (term, weight) pairs, <= 256 together, are sorted by
//            term << 1 | kind: ascending terms, a query entry in front of the selected entry of the same term.  One thread adds
//            F over the selected entries (ascending term) while another adds Q over the query (query order).  Entry i is the
//            head of its term when entry i - 1 has another term; the heads with w > 0 are compacted in order (ballot per wave,
//            wave counts through LDS) into the query's padded row of the workspace.
// srx_feedback_compact_kernel: workgroup b owns the queries [256 b, 256 b + 256).  It adds the row lengths in front of them
//   (integers: any order), scans its own, writes out_ptr, and its waves copy the rows -- an over-long query straight from the
//   input batch -- to their places.
#include "srx_common.h"
#include "ext/sparse_rx_feedback.h"

namespace {

constexpr int FB_MAX_DOCS = SRX_FEEDBACK_MAX_DOCS;
constexpr int FB_MAX_ENTRIES = SRX_FEEDBACK_MAX_ENTRIES;
constexpr int FB_MAX_TERMS = SRX_FEEDBACK_MAX_TERMS;
constexpr int FB_MAX_QTERMS = SRX_FEEDBACK_MAX_QTERMS;
constexpr int FB_ROW = FB_MAX_TERMS + FB_MAX_QTERMS;  // entries of a padded workspace row = the merge's one entry per thread
constexpr int FB_EPT = FB_MAX_ENTRIES / THREADS;      // 16 pairs per thread
constexpr unsigned FB_PAD_KEY = 0xFFFFFFFFu;
static_assert(FB_ROW == THREADS, "the merge holds one entry per thread");
static_assert(FB_MAX_DOCS == 32, "a pair's sort key has 5 bits for the list position");

struct FeedbackArgs {
    const int64_t *row_ptr;
    const int32_t *term;
    const float *value;
    const float *doc_len;    // null under RAW
    const float *term_gain;  // null: 1
    const int32_t *q_ptr, *q_term;
    const float *q_weight;
    const int32_t *fb_doc;
    const float *fb_score;   // null under UNIFORM only
    const int32_t *fb_count; // or null
    int32_t *ws_len;         // [nq]
    int32_t *ws_term;        // [nq][FB_ROW]
    float *ws_weight;        // [nq][FB_ROW]
    int32_t *flag;
    int64_t n_docs, vocab, doc_base;
    int m, fb_docs, row_cap, n_terms, uniform, raw;
    float alpha, beta;
};

struct alignas(16) FeedbackShared {
    unsigned key[FB_MAX_ENTRIES];  // pairs: term << 5 | r.  After the segment sums: unchanged
    float c[FB_MAX_ENTRIES];       // pairs: contribution.  After the segment sums: fb(t) at the head of t's segment
    unsigned hist[RADIX_BINS];
    unsigned ukey[FB_ROW];         // merge: term << 1 | kind (0 = query entry, 1 = selected entry)
    float uval[FB_ROW];            //        the query weight / fb(t)
    unsigned red[16];
    int64_t row_start[FB_MAX_DOCS];
    float row_div[FB_MAX_DOCS];    // doc_len of the row's doc (RM)
    float score[FB_MAX_DOCS];      // the used score, then a_r
    int row_len[FB_MAX_DOCS];      // capped; 0 = not used
    int row_off[FB_MAX_DOCS];      // first pair of the row
    int n_pairs, n_sel, wave_cnt[WAVES];
    float F, Q;
};

__global__ __launch_bounds__(THREADS) void srx_feedback_kernel(FeedbackArgs a) {
    __shared__ FeedbackShared S;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    if (q == 0 && tid == 0) *a.flag = 0;  // the compaction launch sets bit 0
    const int q0 = cload_i32(a.q_ptr + q), nqt = cload_i32(a.q_ptr + q + 1) - q0;
    if (nqt > FB_MAX_QTERMS || nqt < 0) return;  // uniform.  Over-long: the compaction copies the input row (a negative length: an empty row)

    // ---- docs
    if (tid < FB_MAX_DOCS) {
        int limit = a.fb_count != nullptr ? cload_i32(a.fb_count + q) : a.m;
        limit = limit < 0 ? 0 : limit;
        limit = limit > a.m ? a.m : limit;
        limit = limit > a.fb_docs ? a.fb_docs : limit;
        int len = 0;
        int64_t start = 0;
        float sc = 0.0f, div = 1.0f;
        if (tid < limit) {  // tid < m: inside the row
            const int64_t local = (int64_t)gload_i32(a.fb_doc + q * a.m + tid) - a.doc_base;
            bool used = local >= 0 && local < a.n_docs;
            if (!a.uniform) {
                sc = __int_as_float(gload_i32((const int32_t *)a.fb_score + q * a.m + tid));
                used = used && sc > 0.0f && sc < INFINITY;
            }
            if (used) {
                start = ((const SRX_GLOBAL int64_t *)a.row_ptr)[local];
                const int64_t n = ((const SRX_GLOBAL int64_t *)a.row_ptr)[local + 1] - start;
                len = n < 0 ? 0 : n > a.row_cap ? a.row_cap : (int)n;
                if (!a.raw) div = ((const SRX_GLOBAL float *)a.doc_len)[local];
                len |= 0x40000000;  // used, whatever the row's length
            }
        }
        S.row_start[tid] = start, S.row_len[tid] = len, S.score[tid] = sc, S.row_div[tid] = div;
    }
    __syncthreads();
    if (tid == 0) {
        float sum = 0.0f;
        int n_used = 0, off = 0;
        for (int r = 0; r < FB_MAX_DOCS; ++r) {
            const int len = S.row_len[r];
            S.row_off[r] = off;
            if (len != 0) {
                sum = sum + S.score[r];
                ++n_used;
                off += len & 0x3FFFFFFF;  // <= fb_docs * row_cap <= FB_MAX_ENTRIES
            }
        }
        S.n_pairs = off;
        S.n_sel = 0;
        const float each = 1.0f / (float)n_used;
        for (int r = 0; r < FB_MAX_DOCS; ++r) {
            const float s = S.score[r];
            S.score[r] = a.uniform ? each : s / sum;
            S.row_len[r] &= 0x3FFFFFFF;
        }
    }
    __syncthreads();
    const int n_pairs = S.n_pairs;
    int n_sort = 64;
    while (n_sort < n_pairs) n_sort <<= 1;  // <= FB_MAX_ENTRIES

    // ---- gather
    for (int r = wave; r < FB_MAX_DOCS; r += WAVES) {
        const int len = S.row_len[r], off = S.row_off[r];
        const int64_t start = S.row_start[r];
        const float ar = S.score[r], div = S.row_div[r];
        for (int j = lane; j < len; j += 64) {  // off + j < n_pairs <= FB_MAX_ENTRIES
            const int t = gload_i32(a.term + start + j);
            const float v = __int_as_float(gload_i32((const int32_t *)a.value + start + j));
            const float p = a.raw ? v : v / div;
            const bool ok = t >= 0 && t < a.vocab;
            S.key[off + j] = ok ? ((unsigned)t << 5) | (unsigned)r : FB_PAD_KEY;
            S.c[off + j] = ar * p;
        }
    }
    for (int i = n_pairs + tid; i < n_sort; i += THREADS) S.key[i] = FB_PAD_KEY, S.c[i] = 0.0f;
    __syncthreads();

    // ---- sort: ascending by key
    for (int size = 2; size <= n_sort; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int i = tid; i < (n_sort >> 1); i += THREADS) {
                const int pos = 2 * i - (i & (stride - 1));
                const unsigned ka = S.key[pos], kb = S.key[pos + stride];
                const bool asc = (pos & size) == 0;
                if (asc ? (ka > kb) : (ka < kb)) {
                    const float ca = S.c[pos], cb = S.c[pos + stride];
                    S.key[pos] = kb, S.key[pos + stride] = ka;
                    S.c[pos] = cb, S.c[pos + stride] = ca;
                }
            }
            __syncthreads();
        }
    }

    // ---- segment sums and the selection keys of the heads
    unsigned sel[FB_EPT];
    int term[FB_EPT];
    float fb[FB_EPT];
    unsigned mine = 0;
#pragma unroll
    for (int e = 0; e < FB_EPT; ++e) {
        const int i = tid + e * THREADS;
        sel[e] = 0u, term[e] = 0, fb[e] = 0.0f;
        if (i < n_pairs) {
            const unsigned k = S.key[i];
            const unsigned t = k >> 5;
            if (k != FB_PAD_KEY && (i == 0 || (S.key[i - 1] >> 5) != t)) {
                float sum = 0.0f;
                for (int j = i; j < n_pairs && (S.key[j] >> 5) == t; ++j) sum = sum + S.c[j];
                const float g = a.term_gain != nullptr ? ((const SRX_GLOBAL float *)a.term_gain)[t] : 1.0f;  // t < vocab
                if (g > 0.0f && sum > 0.0f) {
                    sel[e] = __float_as_uint(sum * g) + 1u;  // in [1, 0x7F800001]
                    term[e] = (int)t;
                    fb[e] = sum;
                    ++mine;
                }
            }
        }
    }
    const unsigned n_cand = block_sum(mine, S.red);
    TopkCut cut = {0u, 0u};  // keeps every candidate
    if (n_cand > (unsigned)a.n_terms) {  // uniform
        cut = topk_cut((unsigned)a.n_terms, n_cand, [&](auto keys, unsigned k, unsigned n, unsigned *n_gt, unsigned *n_eq) {
            unsigned kk[FB_EPT];
            unsigned mx = 0u, mn = 0xFFFFFFFFu;
#pragma unroll
            for (int e = 0; e < FB_EPT; ++e) {
                kk[e] = sel[e] != 0u ? keys(sel[e], term[e]) : 0u;
                if (kk[e] != 0u) mx = max(mx, kk[e]), mn = min(mn, kk[e]);
            }
            const SumMaxMin r = block_sum_max_min(0u, mx, mn, S.red);
            return radix_kth<FB_EPT>(kk, k, r.mx, r.mn, n, S.hist, S.red, n_gt, n_eq);
        });
    }

    // ---- merge with the query
#pragma unroll
    for (int e = 0; e < FB_EPT; ++e)
        if (cut.keeps(sel[e], term[e])) {
            const int p = atomicAdd(&S.n_sel, 1);  // < n_terms <= FB_MAX_TERMS
            S.ukey[p] = ((unsigned)term[e] << 1) | 1u;
            S.uval[p] = fb[e];
        }
    __syncthreads();
    const int n_sel = S.n_sel, n_union = n_sel + nqt;  // <= FB_ROW
    if (tid >= n_sel) {
        const int j = tid - n_sel;
        const bool in = j < nqt;
        S.ukey[tid] = in ? (unsigned)gload_i32(a.q_term + q0 + j) << 1 : FB_PAD_KEY;
        S.uval[tid] = in ? __int_as_float(gload_i32((const int32_t *)a.q_weight + q0 + j)) : 0.0f;
    }
    __syncthreads();
    for (int size = 2; size <= FB_ROW; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            if (tid < FB_ROW / 2) {
                const int pos = 2 * tid - (tid & (stride - 1));
                const unsigned ka = S.ukey[pos], kb = S.ukey[pos + stride];
                const bool asc = (pos & size) == 0;
                if (asc ? (ka > kb) : (ka < kb)) {
                    const float ca = S.uval[pos], cb = S.uval[pos + stride];
                    S.ukey[pos] = kb, S.ukey[pos + stride] = ka;
                    S.uval[pos] = cb, S.uval[pos + stride] = ca;
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) {  // F: the selected fb in ascending term id
        float sum = 0.0f;
        for (int i = 0; i < n_union; ++i)
            if (S.ukey[i] & 1u) sum = sum + S.uval[i];
        S.F = sum;
    }
    if (tid == 64) {  // Q: the query's weights in query order
        float sum = 0.0f;
        for (int j = 0; j < nqt; ++j) sum = sum + __int_as_float(gload_i32((const int32_t *)a.q_weight + q0 + j));
        S.Q = sum;
    }
    __syncthreads();
    const float F = S.F, Q = S.Q;
    bool emit = false;
    int t_out = 0;
    float w = 0.0f;
    if (tid < n_union) {
        const unsigned k = S.ukey[tid];
        const unsigned t = k >> 1;
        if (tid == 0 || (S.ukey[tid - 1] >> 1) != t) {  // the head of term t: its query entry if it has one
            float A = 0.0f, B = 0.0f;
            int s = tid;                                 // where t's selected entry would be
            if (!(k & 1u)) {
                if (Q > 0.0f) A = a.alpha * (S.uval[tid] / Q);
                s = tid + 1;
                while (s < n_union && (S.ukey[s] >> 1) == t && !(S.ukey[s] & 1u)) ++s;  // a term the query repeats
            }
            if (s < n_union && S.ukey[s] == ((t << 1) | 1u)) B = a.beta * (S.uval[s] / F);
            w = A + B;
            t_out = (int)t;
            emit = w > 0.0f;
        }
    }
    const unsigned long long b = __ballot(emit);
    if (lane == 0) S.wave_cnt[wave] = __popcll(b);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int ww = 0; ww < WAVES; ++ww) {
        if (ww == wave) base = total;
        total += S.wave_cnt[ww];
    }
    if (emit) {
        const int64_t o = q * FB_ROW + base + (int)lane_rank(b);  // base + rank < FB_ROW
        a.ws_term[o] = t_out;
        a.ws_weight[o] = w;
    }
    if (tid == 0) a.ws_len[q] = total;
}

struct CompactArgs {
    const int32_t *q_ptr, *q_term;
    const float *q_weight;
    const int32_t *ws_len, *ws_term;
    const float *ws_weight;
    int32_t *out_ptr, *out_term;
    float *out_weight;
    int32_t *flag;
    int64_t out_capacity;
    int nq;
};

// the length of query q's output row and whether it is the input row copied through
__device__ __forceinline__ int fb_row_len(const CompactArgs &a, int q, bool *through) {
    const int nqt = gload_i32(a.q_ptr + q + 1) - gload_i32(a.q_ptr + q);
    *through = nqt > FB_MAX_QTERMS;
    return *through ? nqt : nqt < 0 ? 0 : gload_i32(a.ws_len + q);
}

__global__ __launch_bounds__(THREADS) void srx_feedback_compact_kernel(CompactArgs a) {
    __shared__ unsigned red[16];
    __shared__ unsigned s_start[THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int qb = blockIdx.x * THREADS;
    bool through;
    unsigned before = 0;
    for (int i = tid; i < qb; i += THREADS) before += (unsigned)fb_row_len(a, i, &through);
    before = block_sum(before, red);
    const int q = qb + tid;
    const unsigned len = q < a.nq ? (unsigned)fb_row_len(a, q, &through) : 0u;
    if (q < a.nq && through) atomicOr((unsigned *)a.flag, 1u);
    unsigned total;
    const unsigned start = before + block_excl_scan(len, red, &total);
    s_start[tid] = start;
    if (q < a.nq) a.out_ptr[q] = (int32_t)start;
    if (q == a.nq - 1) a.out_ptr[a.nq] = (int32_t)(start + len);
    __syncthreads();
    for (int r = wave; r < THREADS && qb + r < a.nq; r += WAVES) {
        const int qq = qb + r;
        const int n = fb_row_len(a, qq, &through);
        const int64_t o = s_start[r];
        const int32_t *src_t = through ? a.q_term + gload_i32(a.q_ptr + qq) : a.ws_term + (int64_t)qq * FB_ROW;
        const float *src_w = through ? a.q_weight + gload_i32(a.q_ptr + qq) : a.ws_weight + (int64_t)qq * FB_ROW;
        for (int j = lane; j < n; j += 64)
            if (o + j < a.out_capacity) {
                a.out_term[o + j] = gload_i32(src_t + j);
                a.out_weight[o + j] = __int_as_float(gload_i32((const int32_t *)src_w + j));
            }
    }
}

int64_t fb_len_words(int64_t nq) { return (nq + 63) / 64 * 64; }

}  // namespace

SRX_API int64_t srx_feedback_workspace_bytes(int32_t nq) {
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", "srx_feedback_workspace_bytes");
    return fb_len_words(nq) * 4 + (int64_t)nq * FB_ROW * 8;
}

SRX_API int srx_feedback_expand(const srx_forward_desc *h_fwd, const srx_feedback_params *h_par, const float *term_gain, const int32_t *q_ptr,
                                const int32_t *q_term, const float *q_weight, int32_t nq, int64_t q_nnz, const int32_t *fb_doc,
                                const float *fb_score, const int32_t *fb_count, int32_t m, int32_t *out_ptr, int32_t *out_term,
                                float *out_weight, int64_t out_capacity, int32_t *flag, void *workspace, int64_t workspace_bytes,
                                void *stream_v) {
    const char *who = "srx_feedback_expand";
    if (!h_fwd) return fail(SRX_ERR_INVALID, "%s: null forward descriptor", who);
    if (!h_par) return fail(SRX_ERR_INVALID, "%s: null params", who);
    const srx_forward_desc &f = *h_fwd;
    const srx_feedback_params &p = *h_par;
    if (f.n_docs < 1 || f.n_docs > 0x7FFFFFFFll - 1) return fail(SRX_ERR_INVALID, "%s: n_docs must be in [1, 2^31 - 2]", who);
    if (f.vocab < 1 || f.vocab > (1ll << 26)) return fail(SRX_ERR_INVALID, "%s: vocab must be in [1, 2^26]", who);
    if (f.doc_base < 0) return fail(SRX_ERR_INVALID, "%s: negative doc_base", who);
    if (f.doc_base >= 0x7FFFFFFFll - f.n_docs) return fail(SRX_ERR_INVALID, "%s: doc_base + n_docs must be below 2^31 - 1", who);
    if (p.fb_docs < 1 || p.fb_docs > FB_MAX_DOCS) return fail(SRX_ERR_INVALID, "%s: fb_docs must be in [1, 32]", who);
    if (p.row_cap < 1) return fail(SRX_ERR_INVALID, "%s: row_cap must be >= 1", who);
    if ((int64_t)p.fb_docs * p.row_cap > FB_MAX_ENTRIES) return fail(SRX_ERR_INVALID, "%s: fb_docs * row_cap must not exceed 4096", who);
    if (p.n_terms < 1 || p.n_terms > FB_MAX_TERMS) return fail(SRX_ERR_INVALID, "%s: n_terms must be in [1, 128]", who);
    if (p.doc_weight != SRX_FB_BY_SCORE && p.doc_weight != SRX_FB_UNIFORM) return fail(SRX_ERR_INVALID, "%s: unknown doc_weight", who);
    if (p.term_weight != SRX_FB_RM && p.term_weight != SRX_FB_RAW) return fail(SRX_ERR_INVALID, "%s: unknown term_weight", who);
    if (p.term_weight == SRX_FB_RM && !f.doc_len) return fail(SRX_ERR_INVALID, "%s: SRX_FB_RM needs doc_len", who);
    if (!(p.alpha >= 0.0f && p.alpha < INFINITY) || !(p.beta >= 0.0f && p.beta < INFINITY))
        return fail(SRX_ERR_INVALID, "%s: alpha and beta must be finite and >= 0", who);
    if (p.alpha == 0.0f && p.beta == 0.0f) return fail(SRX_ERR_INVALID, "%s: alpha and beta are both 0", who);
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if (m < 1) return fail(SRX_ERR_INVALID, "%s: m must be >= 1", who);
    if ((int64_t)nq * m > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: nq * m must not exceed 2^31 - 1", who);
    if (q_nnz < 0 || q_nnz > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: q_nnz must be in [0, 2^31 - 1]", who);
    const int64_t bound = q_nnz + (int64_t)nq * p.n_terms;
    if (bound > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: q_nnz + nq * n_terms must not exceed 2^31 - 1", who);
    if (out_capacity < bound) return fail(SRX_ERR_INVALID, "%s: out_capacity is below q_nnz + nq * n_terms", who);
    if (nq == 0) return SRX_OK;
    if (!f.row_ptr || !f.term || !f.value) return fail(SRX_ERR_INVALID, "%s: null row_ptr / term / value", who);
    if (!q_ptr || (q_nnz > 0 && (!q_term || !q_weight))) return fail(SRX_ERR_INVALID, "%s: null q_ptr / q_term / q_weight", who);
    if (!fb_doc || (p.doc_weight == SRX_FB_BY_SCORE && !fb_score)) return fail(SRX_ERR_INVALID, "%s: null fb_doc / fb_score", who);
    if (!out_ptr || !out_term || !out_weight || !flag) return fail(SRX_ERR_INVALID, "%s: null out_ptr / out_term / out_weight / flag", who);
    if (!workspace || workspace_bytes < srx_feedback_workspace_bytes(nq)) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    HIP_TRY(hipSetDevice(f.device));
    FeedbackArgs a;
    a.row_ptr = f.row_ptr, a.term = f.term, a.value = f.value, a.doc_len = p.term_weight == SRX_FB_RM ? f.doc_len : nullptr;
    a.term_gain = term_gain;
    a.q_ptr = q_ptr, a.q_term = q_term, a.q_weight = q_weight;
    a.fb_doc = fb_doc, a.fb_score = p.doc_weight == SRX_FB_BY_SCORE ? fb_score : nullptr, a.fb_count = fb_count;
    a.ws_len = (int32_t *)workspace;
    a.ws_term = a.ws_len + fb_len_words(nq);
    a.ws_weight = (float *)(a.ws_term + (int64_t)nq * FB_ROW);
    a.flag = flag;
    a.n_docs = f.n_docs, a.vocab = f.vocab, a.doc_base = f.doc_base;
    a.m = m, a.fb_docs = p.fb_docs, a.row_cap = p.row_cap, a.n_terms = p.n_terms;
    a.uniform = p.doc_weight == SRX_FB_UNIFORM, a.raw = p.term_weight == SRX_FB_RAW;
    a.alpha = p.alpha, a.beta = p.beta;
    hipStream_t stream = (hipStream_t)stream_v;
    hipLaunchKernelGGL(srx_feedback_kernel, dim3((unsigned)nq), dim3(THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    CompactArgs c;
    c.q_ptr = q_ptr, c.q_term = q_term, c.q_weight = q_weight;
    c.ws_len = a.ws_len, c.ws_term = a.ws_term, c.ws_weight = a.ws_weight;
    c.out_ptr = out_ptr, c.out_term = out_term, c.out_weight = out_weight;
    c.flag = flag, c.out_capacity = out_capacity, c.nq = nq;
    hipLaunchKernelGGL(srx_feedback_compact_kernel, dim3((unsigned)((nq + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, c);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
