// dense_half_fused.hip -- srx_dense_search_half_fused (include/fused/sparse_rx_half_fused.h): the half-precision search
// without the nq x n_docs score matrix.  The structure is dense_search_i8_impl's (dense.hip) on the half index's 128 x 128
// LDS-staged tile, with filters and the score offset; the pack, GEMM chain and matrix rank kernels are dense_half.hip's,
// compiled here a second time (as tier2_filter.hip compiles tier2_kernel.hip).
//
//   clear      zeroes the pass's counters, overflow flags and thresholds (a kernel, so the call can be captured in a graph).
//   threshold  the first S docs through srx_dense_half_scores_kernel / srx_dense_half_topk_kernel (filter and offset applied),
//              then one wave per query takes the smallest value of a full list as tau[q].
//   screen     hg_block_chain, then per wave and 32 x 32 tile: 16 compares against the thresholds held in LDS, one ballot; a
//              tile without a candidate is done.  A candidate fetches its filter bit, takes a buffer slot by a vector atomic.
//   rank       one workgroup per query that did not overflow folds its buffer (topk_fold); srx_merge_impl ranks the list.
//   fallback   one workgroup per (overflowed query, doc split): a wave scores a 32-row tile with the query in every row of A
//              (the chain of srx_dense_half_score_docs_kernel), lanes 0 .. 31 fold register 0.
// Workgroups keep the grid order of srx_dense_half_scores_kernel (the query blocks of one doc block run together, so the
// doc tiles are read from HBM once and from L2 after that): see DESIGN 4.33.
#define SRX_HALF_SHARED_KERNELS_ONLY  // the query pack, hg_block_chain, the matrix GEMM and the matrix rank: one copy of the text
#include "dense_half.hip"
#include "fused/sparse_rx_half_fused.h"

namespace {

constexpr int HFU_CAP = SRX_HALF_FUSED_CAP;
constexpr int HFU_PASS = SRX_HALF_FUSED_PASS;
constexpr int HFU_CNT_STRIDE = 32;  // ints between two queries' buffer counters: a 128-byte line each (every workgroup of a query block adds to them)
constexpr int HFU_NPT = 16;         // buffer entries per thread and step of the buffer rank
static_assert(SRX_HALF_FUSED_MIN_DOCS <= SRX_HALF_FUSED_CAP, "without a sample every result is kept: the buffer must hold a whole corpus");

// ================================================================================================ clear, threshold
__global__ __launch_bounds__(THREADS) void srx_half_fused_clear_kernel(int *__restrict__ zeroed, int n_zeroed, unsigned *__restrict__ tau, int nq) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i < n_zeroed) zeroed[i] = 0;
    if (i < nq) tau[i] = 0u;
}

// one wave per query: tau = the smallest ranked value of the sample's list if the list is full, else 0
__global__ __launch_bounds__(THREADS) void srx_half_fused_tau_kernel(const float *__restrict__ cand_score, const int32_t *__restrict__ cand_count,
                                                                     int nq, int k, unsigned *__restrict__ tau) {
    const int lane = threadIdx.x & 63, q = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (q >= nq) return;
    const bool full = cand_count[q] >= k;  // the list never holds more than k
    unsigned mn = 0xFFFFFFFFu;
    if (full)
        for (int i = lane; i < k; i += 64) mn = min(mn, __float_as_uint(cand_score[(int64_t)q * k + i]));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mn = min(mn, (unsigned)__shfl_xor((int)mn, off));
    if (lane == 0) tau[q] = full ? mn : 0u;
}

// ================================================================================================ fused GEMM
struct HalfFusedArgs {
    const hf_v4i *corpus, *qpack;
    int64_t n_docs, doc_base;
    int ks, nq, n_qblocks;
    float score_offset;
    const unsigned *tau;        // [nq]
    const uint32_t *fbits;      // may be null
    int64_t fwords;
    const int32_t *q_filter;    // of the pass's first query; may be null
    int32_t *buf_doc;           // [nq][HFU_CAP]
    unsigned *buf_bits;
    int *buf_cnt, *ovf, *any_ovf;
};
template <int TYPE>
__global__ __launch_bounds__(THREADS) void srx_dense_half_fused_kernel(HalfFusedArgs a) {
    __shared__ hg_stage_t stage;
    __shared__ unsigned tau_s[HF_QTILE];  // a query past the pass: no value reaches it
    __shared__ int frow_s[HF_QTILE];      // the query's filter row, -1: not filtered
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int qblock = (int)(blockIdx.x % (unsigned)a.n_qblocks);
    const int64_t dblock = blockIdx.x / (unsigned)a.n_qblocks;
    const int64_t qt0 = (int64_t)qblock * 4, dt0 = dblock * 4;
    if (tid < HF_QTILE) {  // visible behind the chain's barriers
        const int q = qblock * HF_QTILE + tid;
        tau_s[tid] = q < a.nq ? a.tau[q] : 0xFFFFFFFFu;
        frow_s[tid] = (a.fbits != nullptr && q < a.nq) ? (a.q_filter != nullptr ? a.q_filter[q] : 0) : -1;
    }
    hf_v16f acc[2][2];
    hg_block_chain<TYPE>(a.corpus, (a.n_docs + 31) / 32, a.ks, a.qpack, qt0, dt0, stage, acc);
    const int wq = wave >> 1, wd = wave & 1;
    const int64_t d0 = (dt0 + 2 * wd) * 32;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t d = d0 + 32 * j + r;
            const int ql0 = 64 * wq + 32 * i + 4 * h;  // + (reg & 3) + 8 (reg >> 2): the register's query of the block
            float x[16];
            unsigned pass = 0u;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                x[reg] = acc[i][j][reg] + a.score_offset;  // + 0.0f by default (exact)
                const bool keep = x[reg] > 0.0f && __float_as_uint(x[reg]) >= tau_s[ql0 + (reg & 3) + 8 * (reg >> 2)];
                pass |= keep ? 1u << reg : 0u;
            }
            if (d >= a.n_docs) pass = 0u;
            if (__ballot(pass != 0u) == 0ull) continue;  // the usual tile: nothing can reach a top k
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                if ((pass >> reg) & 1u) {
                    const int ql = ql0 + (reg & 3) + 8 * (reg >> 2);
                    const int fr = frow_s[ql];
                    if (fr >= 0 && ((a.fbits[(int64_t)fr * a.fwords + (d >> 5)] >> (d & 31)) & 1u) == 0u) continue;
                    const int q = qblock * HF_QTILE + ql;
                    const int p = atomicAdd(&a.buf_cnt[q * HFU_CNT_STRIDE], 1);
                    if (p < HFU_CAP) {
                        a.buf_doc[(int64_t)q * HFU_CAP + p] = (int)(a.doc_base + d);
                        a.buf_bits[(int64_t)q * HFU_CAP + p] = __float_as_uint(x[reg]);
                    } else {
                        a.ovf[q] = 1;
                        *a.any_ovf = 1;
                    }
                }
        }
}

// ================================================================================================ rank of the buffers
// One workgroup per query: the buffer's entries (all results, all >= tau[q]) folded into an unordered top-k list.  A query
// whose buffer overflowed marks its list (count -1): the merge leaves its row to the fallback.
__global__ __launch_bounds__(THREADS) void srx_half_fused_rank_kernel(const int32_t *__restrict__ buf_doc, const unsigned *__restrict__ buf_bits,
                                                                      const int *__restrict__ buf_cnt, const int *__restrict__ ovf, int k,
                                                                      int32_t *__restrict__ cand_doc, float *__restrict__ cand_score,
                                                                      int32_t *__restrict__ cand_count) {
    __shared__ MergeShared M;
    const int tid = threadIdx.x, q = blockIdx.x;
    if (ovf[q] != 0) {
        if (tid == 0) cand_count[q] = -1;
        return;
    }
    const int total = min(buf_cnt[q * HFU_CNT_STRIDE], HFU_CAP);
    if (tid == 0) {
        M.tk.count = 0;
        M.tk.tau = 0;
    }
    __syncthreads();
    const int32_t *drow = buf_doc + (int64_t)q * HFU_CAP;
    const unsigned *brow = buf_bits + (int64_t)q * HFU_CAP;
    for (int c0 = 0; c0 < total; c0 += THREADS * HFU_NPT) {
        unsigned ubits[HFU_NPT];
        int udoc[HFU_NPT];
        const unsigned tau = M.tk.tau;
#pragma unroll
        for (int n = 0; n < HFU_NPT; ++n) {
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
        topk_fold<HFU_NPT, true>(ubits, udoc, k, M.tk, M.hist);
    }
    __syncthreads();
    topk_shrink(k, M.tk, M.hist);
    const unsigned cnt = M.tk.count;
    for (unsigned i = tid; i < cnt; i += THREADS) {
        cand_doc[(int64_t)q * k + i] = M.tk.doc[i];
        cand_score[(int64_t)q * k + i] = __uint_as_float(M.tk.bits[i]);
    }
    if (tid == 0) cand_count[q] = (int)cnt;
}

// ================================================================================================ exact fallback
struct HalfFallbackArgs {
    const hf_v4i *corpus, *qpack;
    int64_t n_docs, doc_base;
    int ks, k, n_splits;
    float score_offset;
    const uint32_t *fbits;
    int64_t fwords;
    const int32_t *q_filter;
    const int *ovf, *any_ovf;
    int32_t *cand_doc;
    float *cand_score;
    int32_t *cand_count;
};
// Workgroup (query, split): leaves at once unless the query overflowed (its first list is then marked, as the merge of marked
// rows wants it).  Otherwise its four waves walk the split's 32-row tiles, four at a time.
template <int TYPE>
__global__ __launch_bounds__(THREADS) void srx_dense_half_fallback_kernel(HalfFallbackArgs a) {
    __shared__ MergeShared M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    if (*a.any_ovf == 0) return;
    const int q = blockIdx.x / a.n_splits, split = blockIdx.x - q * a.n_splits;
    if (a.ovf[q] == 0) {
        if (tid == 0) a.cand_count[blockIdx.x] = split == 0 ? -1 : 0;
        return;
    }
    const int64_t n_tiles = (a.n_docs + 31) / 32;
    const int64_t t_lo = n_tiles * split / a.n_splits, t_hi = n_tiles * (split + 1) / a.n_splits;
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
    const hf_v4i *qrow = a.qpack + ((int64_t)(q >> 5) * a.ks) * 64 + (q & 31) + 32 * h;  // + 64 per k-step: the query's rounded columns 16 s + 8 h .. + 7
    for (int64_t t0 = t_lo; t0 < t_hi; t0 += WAVES) {  // the same trips for every wave: the fold has barriers
        const int64_t t = t0 + wave;
        const unsigned tau = M.tk.tau;
        unsigned ubits[1] = {0u};
        int udoc[1] = {0};
        if (t < t_hi) {  // wave-uniform
            const hf_v4i *trow = a.corpus + t * a.ks * 64 + lane;
            hf_v16f acc;
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
            for (int s0 = 0; s0 < a.ks; s0 += 4) {  // the search's chain: ascending k from +0.0f; the query is every row of A
                hf_v4i A[4], B[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    A[u] = qrow[(int64_t)(s0 + u) * 64];
                    B[u] = trow[(int64_t)(s0 + u) * 64];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) acc = hf_mfma<TYPE>(A[u], B[u], acc);
            }
            const int64_t d = t * 32 + r;
            const float x = acc[0] + a.score_offset;  // lanes 0 .. 31, register 0: row 0 of the tile, column = doc r
            const unsigned b = __float_as_uint(x);
            if (h == 0 && d < a.n_docs && x > 0.0f && b >= tau && (frow == nullptr || ((frow[d >> 5] >> (d & 31)) & 1u) != 0u)) ubits[0] = b;
            udoc[0] = (int)(a.doc_base + d);
        }
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

// ================================================================================================ host side
// the sample rule of the header
int64_t fused_sample(int64_t n_docs, int k) {
    if (n_docs < SRX_HALF_FUSED_MIN_DOCS) return 0;
    int64_t S = (3 * (int64_t)k * n_docs + HFU_CAP - 1) / HFU_CAP;
    const int64_t floor_s = 164ll * k < 4096 ? 4096 : (164ll * k > 16384 ? 16384 : 164ll * k);
    if (S < floor_s) S = floor_s;
    S = (S + 127) / 128 * 128;
    return S * 4 <= n_docs ? S : 0;
}
struct FusedPlan {
    int qb_max;  // queries of the largest pass
    int64_t S;   // docs of the sample, 0: none
    int L;       // doc splits of the fallback = lists per query of its merge (one merge level, marked rows)
};
FusedPlan fused_plan(int nq, int64_t n_docs, int k) {
    int64_t L = (n_docs + 31) / 32 / 64;
    const int64_t cap = (MERGE_NPT * THREADS) / k < 64 ? (MERGE_NPT * THREADS) / k : 64;
    if (L > cap) L = cap;
    return {nq < HFU_PASS ? nq : HFU_PASS, fused_sample(n_docs, k), (int)(L < 1 ? 1 : L)};
}
struct FusedWs {
    hf_v4i *qpack;
    float *sample;  // [qb_max][S]
    srx_rows cand;  // [qb_max * L] lists of k
    unsigned *tau;
    int *buf_cnt, *ovf, *any_ovf;  // n_zeroed ints
    int n_zeroed;
    int32_t *buf_doc;
    unsigned *buf_bits;
    int64_t bytes;
};
FusedWs fused_ws(void *base, const FusedPlan &pl, int k) {
    const int qb = pl.qb_max;
    FusedWs w;
    char *p = (char *)base;
    auto take = [&](int64_t bytes) {
        char *r = p;
        p += (bytes + 255) / 256 * 256;
        return r;
    };
    w.qpack = (hf_v4i *)take((int64_t)((qb + HF_QTILE - 1) / HF_QTILE) * HF_QTILE * 1024 * 2);  // dim_pad <= 1024
    w.sample = (float *)take((int64_t)qb * pl.S * 4);
    const int64_t lists = (int64_t)qb * pl.L;
    int32_t *cand_doc = (int32_t *)take(lists * k * 4);
    float *cand_score = (float *)take(lists * k * 4);
    w.cand = srx_plain_rows(cand_doc, cand_score, (int32_t *)take(lists * 4), k);
    w.tau = (unsigned *)take((int64_t)qb * 4);
    w.n_zeroed = qb * HFU_CNT_STRIDE + qb + 1;
    w.buf_cnt = (int *)take((int64_t)w.n_zeroed * 4);
    w.ovf = w.buf_cnt + qb * HFU_CNT_STRIDE;
    w.any_ovf = w.ovf + qb;
    w.buf_doc = (int32_t *)take((int64_t)qb * HFU_CAP * 4);
    w.buf_bits = (unsigned *)take((int64_t)qb * HFU_CAP * 4);
    w.bytes = (int64_t)(p - (char *)base) + 256;
    return w;
}

template <int TYPE>
void fused_pass(hipStream_t stream, const FusedPlan &p, const FusedWs &w, const hf_v4i *corpus, int64_t n_docs, int ks, const float *qsrc, int qb,
                int q0, int k, int64_t doc_base, float score_offset, const uint32_t *fbits, const int32_t *qf) {
    const int n_qblocks = (qb + HF_QTILE - 1) / HF_QTILE;
    const int64_t fwords = srx_filter_row_words(n_docs);
    const unsigned pack_grid = (unsigned)(((int64_t)n_qblocks * 4 * ks * 64 + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(srx_half_fused_clear_kernel, dim3((unsigned)((w.n_zeroed + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, w.buf_cnt, w.n_zeroed, w.tau, qb);
    hipLaunchKernelGGL(srx_dense_half_pack_queries_kernel<TYPE>, dim3(pack_grid), dim3(THREADS), 0, stream, qsrc, qb, ks, n_qblocks * 4, w.qpack);
    if (p.S > 0) {  // the threshold: the sample ranked under the filter and the offset
        hipLaunchKernelGGL(srx_dense_half_scores_kernel<TYPE>, dim3((unsigned)(p.S / HF_QTILE * n_qblocks)), dim3(THREADS), 0, stream, corpus, p.S, ks,
                           (const hf_v4i *)w.qpack, qb, n_qblocks, w.sample, p.S);
        hipLaunchKernelGGL(srx_dense_half_topk_kernel, dim3((unsigned)qb), dim3(THREADS), 0, stream, (const float *)w.sample, p.S, p.S, qb, k, 1, doc_base,
                           score_offset, fbits, fwords, qf, q0, w.cand.doc, w.cand.score, w.cand.count);
        hipLaunchKernelGGL(srx_half_fused_tau_kernel, dim3((unsigned)((qb + WAVES - 1) / WAVES)), dim3(THREADS), 0, stream, (const float *)w.cand.score,
                           (const int32_t *)w.cand.count, qb, k, w.tau);
    }
    const int64_t n_dblocks = (n_docs + HF_QTILE - 1) / HF_QTILE;
    const HalfFusedArgs a = {corpus, w.qpack, n_docs, doc_base, ks, qb, n_qblocks, score_offset, w.tau, fbits, fwords, qf != nullptr ? qf + q0 : nullptr,
                             w.buf_doc, w.buf_bits, w.buf_cnt, w.ovf, w.any_ovf};
    hipLaunchKernelGGL(srx_dense_half_fused_kernel<TYPE>, dim3((unsigned)(n_dblocks * n_qblocks)), dim3(THREADS), 0, stream, a);  // <= 2^24 * 8
    hipLaunchKernelGGL(srx_half_fused_rank_kernel, dim3((unsigned)qb), dim3(THREADS), 0, stream, (const int32_t *)w.buf_doc, (const unsigned *)w.buf_bits,
                       (const int *)w.buf_cnt, (const int *)w.ovf, k, w.cand.doc, w.cand.score, w.cand.count);
}
template <int TYPE>
void fused_fallback(hipStream_t stream, const FusedPlan &p, const FusedWs &w, const hf_v4i *corpus, int64_t n_docs, int ks, int qb, int q0, int k,
                    int64_t doc_base, float score_offset, const uint32_t *fbits, const int32_t *qf) {
    const HalfFallbackArgs a = {corpus, w.qpack, n_docs, doc_base, ks, k, p.L, score_offset, fbits, srx_filter_row_words(n_docs),
                                qf != nullptr ? qf + q0 : nullptr, w.ovf, w.any_ovf, w.cand.doc, w.cand.score, w.cand.count};
    hipLaunchKernelGGL(srx_dense_half_fallback_kernel<TYPE>, dim3((unsigned)((int64_t)qb * p.L)), dim3(THREADS), 0, stream, a);
}

}  // namespace

SRX_API int64_t srx_dense_half_fused_workspace_bytes(int32_t nq, int64_t n_docs, int32_t k) {
    if (nq < 0 || n_docs <= 0 || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "srx_dense_half_fused_workspace_bytes: bad argument%s");
    return fused_ws(nullptr, fused_plan(nq, n_docs, k), k).bytes;
}

SRX_API int srx_dense_search_half_fused(int32_t device, int32_t type, const void *corpus_packed, int64_t n_docs, int32_t dim_pad,
                                        const float *queries, int32_t nq, int32_t k, int64_t doc_base, const srx_doc_filter *filter,
                                        int32_t *out_doc, float *out_score, int32_t *out_count, void *workspace, int64_t workspace_bytes,
                                        void *stream_v, float score_offset) {
    const char *who = "srx_dense_search_half_fused";
    if (type != SRX_HALF_F16 && type != SRX_HALF_BF16) return fail(SRX_ERR_INVALID, "%s: type must be SRX_HALF_F16 or SRX_HALF_BF16", who);
    if (filter != nullptr) {
        const int rc = srx_check_filter(who, filter);
        if (rc != SRX_OK) return rc;
    }
    if (nq < 0 || n_docs <= 0 || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "%s: need n_docs > 0, 1 <= k <= 1024", who);
    if (!hf_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 64, <= 1024 (pad the rows with zeros)", who);
    if (doc_base < 0 || doc_base + n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: doc_base + n_docs must fit int32", who);
    if (nq == 0) return SRX_OK;
    if (!corpus_packed || !queries || !out_doc || !out_score || !out_count) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)corpus_packed | (uintptr_t)queries) & 15) return fail(SRX_ERR_INVALID, "%s: corpus / queries must be 16-byte aligned", who);
    const FusedPlan p = fused_plan(nq, n_docs, k);
    const FusedWs w = fused_ws(workspace, p, k);
    if (!workspace || workspace_bytes < w.bytes) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    const int ks = dim_pad / 16;
    const hf_v4i *corpus = (const hf_v4i *)corpus_packed;
    const uint32_t *fbits = filter ? filter->bits : nullptr;
    const int32_t *qf = filter ? filter->q_filter : nullptr;
    for (int q0 = 0; q0 < nq; q0 += HFU_PASS) {
        const int qb = nq - q0 < HFU_PASS ? nq - q0 : HFU_PASS;
        const float *qsrc = queries + (int64_t)q0 * dim_pad;
        const srx_rows out = srx_plain_rows(out_doc + (int64_t)q0 * k, out_score + (int64_t)q0 * k, out_count + q0, k);
        if (type == SRX_HALF_F16)
            fused_pass<SRX_HALF_F16>(stream, p, w, corpus, n_docs, ks, qsrc, qb, q0, k, doc_base, score_offset, fbits, qf);
        else
            fused_pass<SRX_HALF_BF16>(stream, p, w, corpus, n_docs, ks, qsrc, qb, q0, k, doc_base, score_offset, fbits, qf);
        HIP_TRY(hipGetLastError());
        int rc = srx_merge_impl(device, w.cand, qb, 1, k, 0, out, nullptr, 0, stream_v, nullptr, 1);  // the overflowed queries' rows are the fallback's
        if (rc != SRX_OK) return rc;
        if (type == SRX_HALF_F16)
            fused_fallback<SRX_HALF_F16>(stream, p, w, corpus, n_docs, ks, qb, q0, k, doc_base, score_offset, fbits, qf);
        else
            fused_fallback<SRX_HALF_BF16>(stream, p, w, corpus, n_docs, ks, qb, q0, k, doc_base, score_offset, fbits, qf);
        HIP_TRY(hipGetLastError());
        rc = srx_merge_impl(device, w.cand, qb, p.L, k, 0, out, nullptr, 0, stream_v, w.any_ovf, 1);  // behind the same gate; the others are marked
        if (rc != SRX_OK) return rc;
    }
    return SRX_OK;
}
