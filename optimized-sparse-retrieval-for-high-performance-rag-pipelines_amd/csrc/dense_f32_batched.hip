// dense_f32_batched.hip -- srx_dense_search_f32_batched (include/batched/sparse_rx_f32_batched.h): the f32 dense search of a
// query batch.  An fp32 MFMA GEMM screens which (query, doc) pairs can still reach a top k; only those are scored with the
// arithmetic of srx_dense_f32_scores_kernel (dense.hip) / srx_dense_score_docs_f32 (dense_score.hip) and ranked.  Same build
// flags as those units: -ffp-contract=off is what keeps the rescoring bits theirs.
//
//   norm       largest fp32 sum of squares of a row (once per call), by a vector atomic max on the bit pattern.
//   clear      zeroes the pass's counters and overflow flags (a kernel, so the call can be captured in a graph).
//   prep       one wave per query: ||q||_2 and ||q||_1 in fp64 -> the margin m_q and the bound of a query without a threshold.
//   screen     the 128 x 128 tile by v_mfma_f32_32x32x2_f32 through LDS; MATRIX: stores the tile (the threshold sample);
//              otherwise compares against the bounds held in LDS and appends the kept pairs' doc ids to the queries' buffers.
//   tau        one workgroup per query folds the sample's under-estimates into a top-k list: the k-th is tau, and the bound.
//   rescore    one wave per 64 buffer entries: the exact chain, + score_offset, > 0 -> ranked bits next to the ids.
//   rank       one workgroup per query that did not overflow folds its buffer (topk_fold); srx_merge_impl ranks the list.
//   fallback   one workgroup per (overflowed query, doc split): the exact chain over the split's docs, folded directly.
#include "srx_common.h"
#include "filter_common.h"
#include "batched/sparse_rx_f32_batched.h"

namespace {

typedef float fb_v4f __attribute__((ext_vector_type(4)));
typedef float fb_v4u __attribute__((ext_vector_type(4), aligned(4)));  // a 16-byte global load at 4-byte alignment
typedef float fb_v16f __attribute__((ext_vector_type(16)));

constexpr int FB_CAP = SRX_F32_BATCHED_CAP;
constexpr int FB_PASS = SRX_F32_BATCHED_PASS;
constexpr int FB_TILE = 128;        // queries and docs of a workgroup's tile (a wave: 64 x 64)
constexpr int FB_KC = 32;           // columns per chunk staged through LDS
constexpr int FB_LDW = FB_KC + 4;   // floats per LDS row: 16 rows x 36 words cover the 64 banks once
constexpr int FB_CNT_STRIDE = 32;   // ints between two queries' buffer counters: a 128-byte line each
constexpr int FB_NPT = 16;          // entries per thread and step of the folds over a row
constexpr int FB_CHUNKS = FB_CAP / 64;  // waves of the rescore kernel per query
constexpr int FB_FALL_DOCS = THREADS;   // docs per step of a fallback workgroup: 64 per wave
static_assert(SRX_F32_BATCHED_MIN_DOCS <= SRX_F32_BATCHED_CAP, "without a sample every positive pair is kept: the buffer must hold a whole corpus");
static_assert(THREADS == 256 && FB_TILE * FB_KC / 4 == 4 * THREADS, "the staging map: four 16-byte pieces per thread and operand");

// the largest fp32 not above y (y from fp64 arithmetic); a NaN stays one
__device__ __forceinline__ float fb_round_down(double y) {
    float f = (float)y;
    if ((double)f > y) {
        const unsigned b = __float_as_uint(f);
        f = f > 0.0f ? __uint_as_float(b - 1u) : (f == 0.0f ? -1.4e-45f : __uint_as_float(b + 1u));
    }
    return f;
}
// the screen's bound of a query with threshold bits tau (0: none), offset and margin m: the header's inequality chain
__device__ __forceinline__ float fb_bound(unsigned tau, float off, double m) {
    const double tl = tau != 0u ? (double)__uint_as_float(tau - 1u) : 0.0;  // pred(tau)
    return fb_round_down(tl - (double)off - (m + 0x1p-48 * (fabs((double)off) + tl)));
}

// ================================================================================================ norm, clear, prep
__global__ __launch_bounds__(THREADS) void srx_f32_batched_norm_kernel(const float *__restrict__ emb, int64_t n_docs, int dim, unsigned *__restrict__ rsq) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6), n_waves = (int64_t)gridDim.x * WAVES;
    float mx = 0.0f;
    for (int64_t d = wave; d < n_docs; d += n_waves) {
        const float *row = emb + d * dim;
        float s = 0.0f;
        for (int c = lane; c < dim; c += 64) s += row[c] * row[c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        mx = fmaxf(mx, s);
    }
    if (lane == 0) atomicMax(rsq, __float_as_uint(mx));  // sums of squares are >= +0: they order as their bit patterns
}

__global__ __launch_bounds__(THREADS) void srx_f32_batched_clear_kernel(int *__restrict__ zeroed, int n_zeroed) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i < n_zeroed) zeroed[i] = 0;
}

__global__ __launch_bounds__(THREADS) void srx_f32_batched_prep_kernel(const float *__restrict__ queries, int nq, int dim, const unsigned *__restrict__ rsq,
                                                                       float off, double *__restrict__ margin, float *__restrict__ bound) {
    const int lane = threadIdx.x & 63, q = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (q >= nq) return;
    double n2 = 0.0, n1 = 0.0;
    for (int c = lane; c < dim; c += 64) {
        const double x = (double)queries[(int64_t)q * dim + c];
        n2 += x * x;
        n1 += fabs(x);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        n2 += __shfl_xor(n2, o);
        n1 += __shfl_xor(n1, o);
    }
    const double n = (double)dim, nu = n * 0x1p-24, gamma = nu / (1.0 - nu);
    const double R = sqrt((double)__uint_as_float(*rsq)) * (1.0 + 0x1p-9);  // fp32 sum of squares: relative error <= gamma, far inside 2^-9
    const double m = SRX_F32_BATCHED_C * 2.0 * gamma * sqrt(n2) * R * (1.0 + 0x1p-20) + 0x1p-126 * (2.0 * n + n1 + sqrt(n) * R);
    if (lane == 0) {
        margin[q] = m;
        bound[q] = fb_bound(0u, off, m);
    }
}

// ================================================================================================ screen GEMM
struct FbScreenArgs {
    const float *emb, *queries;  // [n_docs][dim]; the pass's [nq][dim]
    int64_t n_docs, doc_base;    // the docs this launch covers: rows 0 .. n_docs - 1
    int dim, nq, n_qblocks;
    const float *bound;          // [nq]: a pair with x~ < bound is dropped
    const uint32_t *fbits;       // may be null
    int64_t fwords;
    const int32_t *q_filter;     // of the pass's first query; may be null
    int32_t *buf_doc;            // [nq][FB_CAP]
    int *buf_cnt, *ovf, *any_ovf;
    float *sample;               // MATRIX: [nq][ld]
    int64_t ld;
};
// Workgroup = (doc block, query block), the query blocks of a doc block adjacent.  Wave w: queries 64 (w >> 1) .., docs 64 (w & 1) ..
// of the tile.  v_mfma_f32_32x32x2_f32 takes from lane l row (l & 31), k (l >> 5) of both operands; D[query][doc]: lane l holds doc
// (l & 31), queries (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).  Staging: thread t moves the 16-byte pieces t, t + 256, .. of each
// operand's 128 x 32 chunk (piece p = row p >> 3, floats 4 (p & 7) ..): eight lanes read 128 contiguous bytes of a row.  Rows past
// the pass / the corpus are clamped to the last one (valid memory, no branch); their accumulators are never looked at.
template <bool MATRIX>
__global__ __launch_bounds__(THREADS) void srx_f32_batched_screen_kernel(FbScreenArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2][2][FB_TILE * FB_LDW];  // [buffer][0: queries, 1: docs]
    __shared__ float bound_s[FB_TILE];
    __shared__ int frow_s[FB_TILE];  // the query's filter row, -1: not filtered
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int qblock = (int)(blockIdx.x % (unsigned)a.n_qblocks);
    const int64_t dblock = blockIdx.x / (unsigned)a.n_qblocks;
    const int q0 = qblock * FB_TILE;
    const int64_t d0 = dblock * FB_TILE;
    if (!MATRIX && tid < FB_TILE) {  // visible behind the chunk loop's barriers
        const int q = q0 + tid;
        bound_s[tid] = q < a.nq ? a.bound[q] : __builtin_inff();
        frow_s[tid] = (a.fbits != nullptr && q < a.nq) ? (a.q_filter != nullptr ? a.q_filter[q] : 0) : -1;
    }
    const float *src[2][4];
    int dst[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int p = tid + THREADS * i, row = p >> 3, c4 = (p & 7) * 4;
        src[0][i] = a.queries + (int64_t)min(q0 + row, a.nq - 1) * a.dim + c4;
        src[1][i] = a.emb + min(d0 + row, a.n_docs - 1) * a.dim + c4;
        dst[i] = row * FB_LDW + c4;
    }
    fb_v4f stg[2][4];
    auto fetch = [&](int c) __attribute__((always_inline)) {
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int i = 0; i < 4; ++i) stg[o][i] = *reinterpret_cast<const fb_v4u *>(src[o][i] + c * FB_KC);
    };
    auto put = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int i = 0; i < 4; ++i) *reinterpret_cast<fb_v4f *>(&lds[buf][o][dst[i]]) = stg[o][i];
    };
    fb_v16f acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][t][e] = 0.0f;
    const int wq = wave >> 1, wd = wave & 1;
    const int a_off = (64 * wq + r) * FB_LDW + 4 * h, b_off = (64 * wd + r) * FB_LDW + 4 * h;
    const int n_chunks = a.dim / FB_KC;
    fetch(0);
    put(0);
    __syncthreads();
    for (int c = 0; c < n_chunks; ++c) {
        const int buf = c & 1;
        if (c + 1 < n_chunks) fetch(c + 1);  // in flight during this chunk's MFMAs
#pragma unroll
        for (int j = 0; j < FB_KC / 8; ++j) {  // a 16-byte read = the lane's operand of four k-steps (columns 8 j + 4 h ..)
            fb_v4f A[2], B[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                A[i] = *reinterpret_cast<const fb_v4f *>(&lds[buf][0][a_off + 32 * i * FB_LDW + 8 * j]);
                B[i] = *reinterpret_cast<const fb_v4f *>(&lds[buf][1][b_off + 32 * i * FB_LDW + 8 * j]);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int t = 0; t < 2; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[i][e], B[t][e], acc[i][t], 0, 0, 0);
        }
        if (c + 1 < n_chunks) put(buf ^ 1);  // that buffer was last read in chunk c - 1: one barrier ago
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int64_t d = d0 + 64 * wd + 32 * t + r;
            const int ql0 = 64 * wq + 32 * i + 4 * h;  // + (reg & 3) + 8 (reg >> 2): the register's query of the block
            if constexpr (MATRIX) {
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int q = q0 + ql0 + (reg & 3) + 8 * (reg >> 2);
                    if (q < a.nq && d < a.n_docs) a.sample[(int64_t)q * a.ld + d] = acc[i][t][reg];
                }
            } else {
                unsigned pass = 0u;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)  // "not below": a NaN goes to the exact arithmetic
                    pass |= !(acc[i][t][reg] < bound_s[ql0 + (reg & 3) + 8 * (reg >> 2)]) ? 1u << reg : 0u;
                if (d >= a.n_docs) pass = 0u;
                if (__ballot(pass != 0u) == 0ull) continue;  // the usual tile: nothing can reach a top k
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    if ((pass >> reg) & 1u) {
                        const int ql = ql0 + (reg & 3) + 8 * (reg >> 2), q = q0 + ql;
                        if (q >= a.nq) continue;  // a clamped copy of the last query
                        const int fr = frow_s[ql];
                        if (fr >= 0 && ((a.fbits[(int64_t)fr * a.fwords + (d >> 5)] >> (d & 31)) & 1u) == 0u) continue;
                        const int p = atomicAdd(&a.buf_cnt[q * FB_CNT_STRIDE], 1);
                        if (p < FB_CAP) {
                            a.buf_doc[(int64_t)q * FB_CAP + p] = (int)(a.doc_base + d);
                        } else {
                            a.ovf[q] = 1;
                            *a.any_ovf = 1;
                        }
                    }
            }
        }
}

// ================================================================================================ threshold
// One workgroup per query over its row of the sample matrix.  An allowed doc counts with y = rd32(x~ + offset - m - fp64 slack):
// not above its exact ranked value.  The k-th best y (0 without k of them) is tau; the bound follows.
__global__ __launch_bounds__(THREADS) void srx_f32_batched_tau_kernel(const float *__restrict__ sample, int64_t S, int k, float off,
                                                                      const double *__restrict__ margin, const uint32_t *__restrict__ fbits,
                                                                      int64_t fwords, const int32_t *__restrict__ q_filter, float *__restrict__ bound) {
    __shared__ MergeShared M;
    const int tid = threadIdx.x, q = blockIdx.x;
    const uint32_t *frow = nullptr;
    if (fbits != nullptr) {
        const int fr = q_filter != nullptr ? q_filter[q] : 0;
        if (fr >= 0) frow = fbits + (int64_t)fr * fwords;
    }
    if (tid == 0) {
        M.tk.count = 0;
        M.tk.tau = 0;
    }
    __syncthreads();
    const double m = margin[q];
    const float *row = sample + (int64_t)q * S;
    for (int64_t c0 = 0; c0 < S; c0 += (int64_t)THREADS * FB_NPT) {
        unsigned ubits[FB_NPT];
        int udoc[FB_NPT];
        const unsigned tau = M.tk.tau;
#pragma unroll
        for (int n = 0; n < FB_NPT; ++n) {
            const int64_t c = c0 + (int64_t)n * THREADS + tid;
            float y = 0.0f;
            if (c < S && (frow == nullptr || ((frow[c >> 5] >> (c & 31)) & 1u) != 0u)) {
                const double x = (double)row[c];
                y = fb_round_down(x + (double)off - (m + 0x1p-48 * (fabs((double)off) + fabs(x))));
            }
            const unsigned b = __float_as_uint(y);
            ubits[n] = (y > 0.0f && b >= tau) ? b : 0u;  // a NaN does not count
            udoc[n] = (int)c;
        }
        topk_fold<FB_NPT, true>(ubits, udoc, k, M.tk, M.hist);
    }
    __syncthreads();
    topk_shrink(k, M.tk, M.hist);
    const unsigned cnt = M.tk.count;
    unsigned mn = 0xFFFFFFFFu;
    for (unsigned i = tid; i < cnt; i += THREADS) mn = min(mn, M.tk.bits[i]);
    const SumMaxMin rr = block_sum_max_min(0u, 0u, mn, M.tk.red);
    if (tid == 0) bound[q] = fb_bound(cnt >= (unsigned)k ? rr.mn : 0u, off, m);
}

// ================================================================================================ exact arithmetic
// The scores of the wave's 64 rows (lane j: row `row`, < 0: none) against the query held as qv (lane l: columns l, l + 64, ..):
// the chain of srx_dense_f32_scores_kernel -- products summed in ascending slice order from +0, then the xor butterfly.  Slices
// beyond dim are zeros on both sides and change no bit.  U rows are loaded before the first is used.
template <int NS, int U>
__device__ __forceinline__ float fb_exact_scores(const float *__restrict__ emb, int dim, int row, const float (&qv)[NS]) {
    const int lane = threadIdx.x & 63, ns = dim >> 6;
    const unsigned long long live = __ballot(row >= 0);
    float res = 0.0f;
    for (int c0 = 0; c0 < 64; c0 += U) {
        if (((live >> c0) & ((1ull << U) - 1ull)) == 0ull) continue;  // uniform
        float rv[U][NS];
        int rw[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            rw[u] = __shfl(row, c0 + u);
            const float *p = emb + (int64_t)rw[u] * dim;
#pragma unroll
            for (int i = 0; i < NS; ++i) rv[u][i] = (rw[u] >= 0 && i < ns) ? p[lane + 64 * i] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float s = 0.0f;
#pragma unroll
            for (int i = 0; i < NS; ++i) s = s + rv[u][i] * qv[i];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
            if (lane == c0 + u && rw[u] >= 0) res = s;  // every lane holds the same bits
        }
    }
    return res;
}
template <int NS>
__device__ __forceinline__ void fb_load_query(const float *__restrict__ qrow, int dim, float (&qv)[NS]) {
    const int lane = threadIdx.x & 63, ns = dim >> 6;
#pragma unroll
    for (int i = 0; i < NS; ++i) qv[i] = i < ns ? qrow[lane + 64 * i] : 0.0f;
}

struct FbExactArgs {
    const float *emb, *queries;
    int64_t n_docs, doc_base;
    int dim, nq, k, n_splits;
    float score_offset;
    const uint32_t *fbits;
    int64_t fwords;
    const int32_t *q_filter;
    const int32_t *buf_doc;
    unsigned *buf_bits;
    const int *buf_cnt, *ovf, *any_ovf;
    int32_t *cand_doc;
    float *cand_score;
    int32_t *cand_count;
};

// One wave per (query, 64 buffer entries): ranked bits of fl32(score + offset) > 0, else 0, next to the ids
template <int NS, int U>
__global__ __launch_bounds__(THREADS) void srx_f32_batched_rescore_kernel(FbExactArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    const int q = (int)(w / FB_CHUNKS), c = (int)(w % FB_CHUNKS) * 64 + lane;
    if (q >= a.nq || a.ovf[q] != 0) return;  // an overflowed query is the fallback's
    const int total = min(a.buf_cnt[q * FB_CNT_STRIDE], FB_CAP);
    if (c - lane >= total) return;  // whole waves leave
    const int row = c < total ? (int)((int64_t)a.buf_doc[(int64_t)q * FB_CAP + c] - a.doc_base) : -1;
    float qv[NS];
    fb_load_query<NS>(a.queries + (int64_t)q * a.dim, a.dim, qv);
    const float x = fb_exact_scores<NS, U>(a.emb, a.dim, row, qv) + a.score_offset;  // + 0.0f by default (exact)
    if (c < total) a.buf_bits[(int64_t)q * FB_CAP + c] = x > 0.0f ? __float_as_uint(x) : 0u;
}

// One workgroup per query: the buffer's entries folded into an unordered top-k list.  A query whose buffer overflowed marks its
// list (count -1): the merge leaves its row to the fallback.
__global__ __launch_bounds__(THREADS) void srx_f32_batched_rank_kernel(FbExactArgs a) {
    __shared__ MergeShared M;
    const int tid = threadIdx.x, q = blockIdx.x;
    if (a.ovf[q] != 0) {
        if (tid == 0) a.cand_count[q] = -1;
        return;
    }
    const int total = min(a.buf_cnt[q * FB_CNT_STRIDE], FB_CAP);
    if (tid == 0) {
        M.tk.count = 0;
        M.tk.tau = 0;
    }
    __syncthreads();
    const int32_t *drow = a.buf_doc + (int64_t)q * FB_CAP;
    const unsigned *brow = a.buf_bits + (int64_t)q * FB_CAP;
    for (int c0 = 0; c0 < total; c0 += THREADS * FB_NPT) {
        unsigned ubits[FB_NPT];
        int udoc[FB_NPT];
        const unsigned tau = M.tk.tau;
#pragma unroll
        for (int n = 0; n < FB_NPT; ++n) {
            const int c = c0 + n * THREADS + tid;
            unsigned b = 0u;
            int dd = 0;
            if (c < total) {
                b = brow[c];
                dd = drow[c];
            }
            ubits[n] = b >= tau ? b : 0u;
            udoc[n] = dd;
        }
        topk_fold<FB_NPT, true>(ubits, udoc, a.k, M.tk, M.hist);
    }
    __syncthreads();
    topk_shrink(a.k, M.tk, M.hist);
    const unsigned cnt = M.tk.count;
    for (unsigned i = tid; i < cnt; i += THREADS) {
        a.cand_doc[(int64_t)q * a.k + i] = M.tk.doc[i];
        a.cand_score[(int64_t)q * a.k + i] = __uint_as_float(M.tk.bits[i]);
    }
    if (tid == 0) a.cand_count[q] = (int)cnt;
}

// Workgroup (query, split): leaves at once unless the query overflowed (its first list is then marked, as the merge of marked rows
// wants it).  Otherwise its four waves walk the split's docs, 64 per wave and step, and fold one value per thread.
template <int NS, int U>
__global__ __launch_bounds__(THREADS) void srx_f32_batched_fallback_kernel(FbExactArgs a) {
    __shared__ MergeShared M;
    const int tid = threadIdx.x;
    if (*a.any_ovf == 0) return;
    const int q = blockIdx.x / a.n_splits, split = blockIdx.x - q * a.n_splits;
    if (a.ovf[q] == 0) {
        if (tid == 0) a.cand_count[blockIdx.x] = split == 0 ? -1 : 0;
        return;
    }
    const int64_t n_steps = (a.n_docs + FB_FALL_DOCS - 1) / FB_FALL_DOCS;
    const int64_t s_lo = n_steps * split / a.n_splits, s_hi = n_steps * (split + 1) / a.n_splits;
    const uint32_t *frow = nullptr;
    if (a.fbits != nullptr) {
        const int fr = a.q_filter != nullptr ? a.q_filter[q] : 0;
        if (fr >= 0) frow = a.fbits + (int64_t)fr * a.fwords;
    }
    if (tid == 0) {
        M.tk.count = 0;
        M.tk.tau = 0;
    }
    __syncthreads();
    float qv[NS];
    fb_load_query<NS>(a.queries + (int64_t)q * a.dim, a.dim, qv);
    for (int64_t s = s_lo; s < s_hi; ++s) {  // the same trips for every wave: the fold has barriers
        const int64_t d = s * FB_FALL_DOCS + tid;
        const bool on = d < a.n_docs && (frow == nullptr || ((frow[d >> 5] >> (d & 31)) & 1u) != 0u);
        const float x = fb_exact_scores<NS, U>(a.emb, a.dim, on ? (int)d : -1, qv) + a.score_offset;
        const unsigned tau = M.tk.tau, b = __float_as_uint(x);
        unsigned ubits[1] = {(on && x > 0.0f && b >= tau) ? b : 0u};
        int udoc[1] = {(int)(a.doc_base + d)};
        topk_fold<1, true>(ubits, udoc, a.k, M.tk, M.hist);
    }
    __syncthreads();
    topk_shrink(a.k, M.tk, M.hist);
    const unsigned cnt = M.tk.count;
    const int64_t o = (int64_t)blockIdx.x * a.k;
    for (unsigned i = tid; i < cnt; i += THREADS) {
        a.cand_doc[o + i] = M.tk.doc[i];
        a.cand_score[o + i] = __uint_as_float(M.tk.bits[i]);
    }
    if (tid == 0) a.cand_count[blockIdx.x] = (int)cnt;
}

#ifndef SRX_F32_BATCHED_KERNELS_ONLY  // tools/f32_mfma_probe.hip compiles the kernels above alone
// ================================================================================================ host side
// the sample rule of the header
int64_t fb_sample(int64_t n_docs, int k) {
    if (n_docs < SRX_F32_BATCHED_MIN_DOCS) return 0;
    int64_t S = ((int64_t)k * n_docs + SRX_F32_BATCHED_TARGET - 1) / SRX_F32_BATCHED_TARGET;
    const int64_t floor_s = 164ll * k < 4096 ? 4096 : (164ll * k > 16384 ? 16384 : 164ll * k);
    if (S < floor_s) S = floor_s;
    if (S > SRX_F32_BATCHED_MAX_SAMPLE) S = SRX_F32_BATCHED_MAX_SAMPLE;
    S = (S + 127) / 128 * 128;
    return S * 4 <= n_docs ? S : 0;
}
struct FbPlan {
    int qb_max;  // queries of the largest pass
    int64_t S;   // docs of the sample, 0: none
    int L;       // doc splits of the fallback = lists per query of its merge (one merge level, marked rows)
};
FbPlan fb_plan(int nq, int64_t n_docs, int k) {
    int64_t L = (n_docs + FB_FALL_DOCS - 1) / FB_FALL_DOCS / 16;
    const int64_t cap = (MERGE_NPT * THREADS) / k < 64 ? (MERGE_NPT * THREADS) / k : 64;
    if (L > cap) L = cap;
    return {nq < FB_PASS ? nq : FB_PASS, fb_sample(n_docs, k), (int)(L < 1 ? 1 : L)};
}
struct FbWs {
    unsigned *rsq;
    double *margin;
    float *bound;
    float *sample;  // [qb_max][S]
    srx_rows cand;  // [qb_max * L] lists of k
    int *buf_cnt, *ovf, *any_ovf;  // n_zeroed ints
    int n_zeroed;
    int32_t *buf_doc;
    unsigned *buf_bits;
    int64_t bytes;
};
FbWs fb_ws(void *base, const FbPlan &pl, int k) {
    const int qb = pl.qb_max;
    FbWs w;
    char *p = (char *)base;
    auto take = [&](int64_t bytes) {
        char *r = p;
        p += (bytes + 255) / 256 * 256;
        return r;
    };
    w.rsq = (unsigned *)take(256);
    w.margin = (double *)take((int64_t)qb * 8);
    w.bound = (float *)take((int64_t)qb * 4);
    w.sample = (float *)take((int64_t)qb * pl.S * 4);
    const int64_t lists = (int64_t)qb * pl.L;
    int32_t *cand_doc = (int32_t *)take(lists * k * 4);
    float *cand_score = (float *)take(lists * k * 4);
    w.cand = srx_plain_rows(cand_doc, cand_score, (int32_t *)take(lists * 4), k);
    w.n_zeroed = qb * FB_CNT_STRIDE + qb + 1;
    w.buf_cnt = (int *)take((int64_t)w.n_zeroed * 4);
    w.ovf = w.buf_cnt + qb * FB_CNT_STRIDE;
    w.any_ovf = w.ovf + qb;
    w.buf_doc = (int32_t *)take((int64_t)qb * FB_CAP * 4);
    w.buf_bits = (unsigned *)take((int64_t)qb * FB_CAP * 4);
    w.bytes = (int64_t)(p - (char *)base) + 256;
    return w;
}

// f(IntC<NS>, IntC<U>) for the bucket of slices that holds dim / 64 (the buckets of dense_score.hip)
template <typename F>
void fb_for_slices(int dim, F &&f) {
    const int ns = dim >> 6;
    if (ns <= 1) f(IntC<1>{}, IntC<8>{});
    else if (ns <= 2) f(IntC<2>{}, IntC<8>{});
    else if (ns <= 4) f(IntC<4>{}, IntC<8>{});
    else if (ns <= 8) f(IntC<8>{}, IntC<8>{});
    else f(IntC<16>{}, IntC<4>{});
}
}  // namespace

SRX_API int64_t srx_dense_f32_batched_workspace_bytes(int32_t nq, int64_t n_docs, int32_t k) {
    if (nq < 0 || n_docs <= 0 || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "srx_dense_f32_batched_workspace_bytes: bad argument%s");
    return fb_ws(nullptr, fb_plan(nq, n_docs, k), k).bytes;
}

SRX_API int srx_dense_search_f32_batched(int32_t device, const float *emb, int64_t n_docs, int32_t dim, const float *queries, int32_t nq,
                                         int32_t k, int64_t doc_base, const srx_doc_filter *filter, int32_t *out_doc, float *out_score,
                                         int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream_v, float score_offset) {
    const char *who = "srx_dense_search_f32_batched";
    if (filter != nullptr) {
        const int rc = srx_check_filter(who, filter);
        if (rc != SRX_OK) return rc;
    }
    if (nq < 0 || n_docs <= 0 || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "%s: need n_docs > 0, 1 <= k <= 1024", who);
    if (dim <= 0 || dim % 64 != 0 || dim > 1024) return fail(SRX_ERR_INVALID, "%s: dim must be a multiple of 64, <= 1024 (pad the rows with zeros)", who);
    if (doc_base < 0 || doc_base + n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: doc_base + n_docs must fit int32", who);
    if (nq == 0) return SRX_OK;
    if (!emb || !queries || !out_doc || !out_score || !out_count) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    const FbPlan p = fb_plan(nq, n_docs, k);
    const FbWs w = fb_ws(workspace, p, k);
    if (!workspace || workspace_bytes < w.bytes) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    const uint32_t *fbits = filter ? filter->bits : nullptr;
    const int32_t *qf = filter ? filter->q_filter : nullptr;
    const int64_t fwords = srx_filter_row_words(n_docs);
    // R, once per call
    int64_t norm_blocks = (n_docs + WAVES - 1) / WAVES;
    if (norm_blocks > 256 * 16) norm_blocks = 256 * 16;
    hipLaunchKernelGGL(srx_f32_batched_clear_kernel, dim3(1), dim3(THREADS), 0, stream, (int *)w.rsq, 1);
    hipLaunchKernelGGL(srx_f32_batched_norm_kernel, dim3((unsigned)norm_blocks), dim3(THREADS), 0, stream, emb, n_docs, (int)dim, w.rsq);
    for (int q0 = 0; q0 < nq; q0 += FB_PASS) {
        const int qb = nq - q0 < FB_PASS ? nq - q0 : FB_PASS;
        const float *qsrc = queries + (int64_t)q0 * dim;
        const int32_t *qfp = qf != nullptr ? qf + q0 : nullptr;
        const srx_rows out = srx_plain_rows(out_doc + (int64_t)q0 * k, out_score + (int64_t)q0 * k, out_count + q0, k);
        const int n_qblocks = (qb + FB_TILE - 1) / FB_TILE;
        hipLaunchKernelGGL(srx_f32_batched_clear_kernel, dim3((unsigned)((w.n_zeroed + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, w.buf_cnt, w.n_zeroed);
        hipLaunchKernelGGL(srx_f32_batched_prep_kernel, dim3((unsigned)((qb + WAVES - 1) / WAVES)), dim3(THREADS), 0, stream, qsrc, qb, (int)dim,
                           (const unsigned *)w.rsq, score_offset, w.margin, w.bound);
        FbScreenArgs s = {emb, qsrc, n_docs, doc_base, (int)dim, qb, n_qblocks, w.bound, fbits, fwords, qfp, w.buf_doc, w.buf_cnt, w.ovf, w.any_ovf, w.sample, p.S};
        if (p.S > 0) {  // the threshold: the sample's under-estimates ranked under the filter and the offset
            FbScreenArgs m = s;
            m.n_docs = p.S;
            hipLaunchKernelGGL(srx_f32_batched_screen_kernel<true>, dim3((unsigned)(p.S / FB_TILE * n_qblocks)), dim3(THREADS), 0, stream, m);
            hipLaunchKernelGGL(srx_f32_batched_tau_kernel, dim3((unsigned)qb), dim3(THREADS), 0, stream, (const float *)w.sample, p.S, (int)k, score_offset,
                               (const double *)w.margin, fbits, fwords, qfp, w.bound);
        }
        const int64_t n_dblocks = (n_docs + FB_TILE - 1) / FB_TILE;
        hipLaunchKernelGGL(srx_f32_batched_screen_kernel<false>, dim3((unsigned)(n_dblocks * n_qblocks)), dim3(THREADS), 0, stream, s);  // <= 2^24 * 8
        const FbExactArgs e = {emb, qsrc, n_docs, doc_base, (int)dim, qb, (int)k, p.L, score_offset, fbits, fwords, qfp, w.buf_doc, w.buf_bits,
                               w.buf_cnt, w.ovf, w.any_ovf, w.cand.doc, w.cand.score, w.cand.count};
        fb_for_slices(dim, [&](auto NS, auto U) {
            hipLaunchKernelGGL((srx_f32_batched_rescore_kernel<decltype(NS)::value, decltype(U)::value>), dim3((unsigned)((int64_t)qb * FB_CHUNKS / WAVES)),
                               dim3(THREADS), 0, stream, e);
        });
        hipLaunchKernelGGL(srx_f32_batched_rank_kernel, dim3((unsigned)qb), dim3(THREADS), 0, stream, e);
        HIP_TRY(hipGetLastError());
        int rc = srx_merge_impl(device, w.cand, qb, 1, k, 0, out, nullptr, 0, stream_v, nullptr, 1);  // the overflowed queries' rows are the fallback's
        if (rc != SRX_OK) return rc;
        fb_for_slices(dim, [&](auto NS, auto U) {
            hipLaunchKernelGGL((srx_f32_batched_fallback_kernel<decltype(NS)::value, decltype(U)::value>), dim3((unsigned)((int64_t)qb * p.L)), dim3(THREADS), 0,
                               stream, e);
        });
        HIP_TRY(hipGetLastError());
        rc = srx_merge_impl(device, w.cand, qb, p.L, k, 0, out, nullptr, 0, stream_v, w.any_ovf, 1);  // behind the same gate; the others are marked
        if (rc != SRX_OK) return rc;
    }
    return SRX_OK;
}
#else
}  // namespace
#endif
