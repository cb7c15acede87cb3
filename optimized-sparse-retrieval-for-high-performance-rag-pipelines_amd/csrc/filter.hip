// filter.hip -- the doc filters of sparse_rx_filter.h: building, editing and counting filter rows (one bit per shard-local doc),
// the checks of a filter that every filtered search shares, and the dense side's row ranking under a filter.  The sparse search
// tests the bits where it forms its candidates: tier2_filter.hip (after_bound).
//
// Replaces nothing in the reference project: it has no filters.

#include "filter_common.h"

namespace {
constexpr unsigned FILTER_MAX_GRID = 256 * 16;          // grid-stride loops: 16 workgroups per CU at most

// Every word of every row: ones below n_docs when value is set, zeros above and in the padding words.
__global__ __launch_bounds__(THREADS) void srx_filter_fill_kernel(uint32_t *__restrict__ bits, int64_t total_words, int64_t words,
                                                                  int64_t n_docs, int value) {
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < total_words; i += (int64_t)gridDim.x * THREADS) {
        const int64_t first = (i % words) * 32;  // the word's first doc
        uint32_t w = 0u;
        if (value && first < n_docs) w = n_docs - first >= 32 ? 0xFFFFFFFFu : (1u << (int)(n_docs - first)) - 1u;
        bits[i] = w;
    }
}

// One thread per listed id: ids outside the shard (-1 padding, other shards' docs) are skipped; duplicates hit the same bit.
__global__ __launch_bounds__(THREADS) void srx_filter_set_docs_kernel(uint32_t *__restrict__ row, int64_t n_docs, int64_t doc_base,
                                                                      const int32_t *__restrict__ doc, int64_t n, int value) {
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const int64_t d = (int64_t)doc[i] - doc_base;
        if (d < 0 || d >= n_docs) continue;
        const uint32_t bit = 1u << (int)(d & 31);
        if (value)
            atomicOr(&row[d >> 5], bit);
        else
            atomicAnd(&row[d >> 5], ~bit);
    }
}

// One workgroup per row: popcount of its doc bits (the tail of the last word is masked, whatever it holds).
__global__ __launch_bounds__(THREADS) void srx_filter_count_kernel(const uint32_t *__restrict__ bits, int64_t words, int64_t n_docs,
                                                                   int32_t *__restrict__ out_count) {
    __shared__ unsigned red[16];
    const uint32_t *row = bits + (int64_t)blockIdx.x * words;
    const int64_t used = (n_docs + 31) / 32;
    unsigned mine = 0;
    for (int64_t i = threadIdx.x; i < used; i += THREADS) {
        uint32_t w = row[i];
        if (n_docs - i * 32 < 32) w &= (1u << (int)(n_docs - i * 32)) - 1u;
        mine += (unsigned)__popc(w);
    }
    const unsigned total = block_sum(mine, red);
    if (threadIdx.x == 0) out_count[blockIdx.x] = (int32_t)total;
}

// The dense side's row ranking under a filter: one workgroup per (query, split of the columns) folds the allowed columns of its
// slice of the score row into an exact lazy top-k list, as srx_dense_topk_kernel (dense.hip) does with all of them.  Column c
// is ranked iff bit c & 31 of word c >> 5 of the query's row is set: consecutive lanes read consecutive bits, 32 lanes a word.
constexpr int FILTER_NPT = 16;  // columns per thread and step (dense.hip: DENSE_NPT)
__global__ __launch_bounds__(THREADS) void srx_filtered_topk_kernel(const float *__restrict__ scores, int64_t ld, int64_t n_docs, int nq,
                                                                    int k, int n_splits, int64_t doc_base,
                                                                    const uint32_t *__restrict__ filter_bits, int64_t filter_words,
                                                                    const int32_t *__restrict__ q_filter, int q0,
                                                                    int32_t *__restrict__ cand_doc, float *__restrict__ cand_score,
                                                                    int32_t *__restrict__ cand_count) {
    __shared__ MergeShared M;
    const int tid = threadIdx.x;
    const int q = blockIdx.x / n_splits, split = blockIdx.x - q * n_splits;
    if (q >= nq) return;
    const int64_t lo = n_docs * split / n_splits, hi = n_docs * (split + 1) / n_splits;
    const int r = q_filter != nullptr ? q_filter[q0 + q] : 0;
    const uint32_t *frow = r >= 0 ? filter_bits + (int64_t)r * filter_words : nullptr;  // null: this query is not filtered
    if (tid == 0) {
        M.tk.count = 0;
        M.tk.tau = 0;
    }
    __syncthreads();
    const float *row = scores + (int64_t)q * ld;
    for (int64_t c0 = lo; c0 < hi; c0 += (int64_t)THREADS * FILTER_NPT) {
        unsigned ubits[FILTER_NPT];
        int udoc[FILTER_NPT];
        const unsigned tau = M.tk.tau;
#pragma unroll
        for (int n = 0; n < FILTER_NPT; ++n) {
            const int64_t c = c0 + (int64_t)n * THREADS + tid;
            float x = 0.0f;
            bool allowed = false;
            if (c < hi) {  // c < n_docs: the row has a word for it
                x = row[c];
                allowed = frow == nullptr || ((frow[c >> 5] >> (c & 31)) & 1u) != 0u;
            }
            const unsigned b = __float_as_uint(x);
            ubits[n] = (allowed && x > 0.0f && b >= tau) ? b : 0u;
            udoc[n] = (int)(doc_base + c);
        }
        topk_fold<FILTER_NPT, true>(ubits, udoc, k, M.tk, M.hist);
    }
    __syncthreads();
    topk_shrink(k, M.tk, M.hist);
    const unsigned cnt = M.tk.count;
    const int64_t o = (int64_t)blockIdx.x * k;
    for (unsigned i = tid; i < cnt; i += THREADS) {
        cand_doc[o + i] = M.tk.doc[i];
        cand_score[o + i] = __uint_as_float(M.tk.bits[i]);
    }
    if (tid == 0) cand_count[blockIdx.x] = (int)cnt;
}

int check_rows(const char *who, const void *bits, int64_t n_docs) {
    if (n_docs < 1 || n_docs > SRX_FILTER_MAX_DOCS) return fail(SRX_ERR_INVALID, "%s: n_docs must be in [1, 2^31 - 2]", who);
    if (!bits) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)bits & 15) return fail(SRX_ERR_INVALID, "%s: filter rows must be 16-byte aligned", who);
    return SRX_OK;
}
unsigned grid_for(int64_t items) {
    const int64_t g = (items + THREADS - 1) / THREADS;
    return (unsigned)(g < 1 ? 1 : g > FILTER_MAX_GRID ? FILTER_MAX_GRID : g);
}
}  // namespace

int srx_check_filter(const char *who, const srx_doc_filter *f) {
    if (!f) return fail(SRX_ERR_INVALID, "%s: null filter", who);
    if (!f->bits) return fail(SRX_ERR_INVALID, "%s: null filter bits", who);
    if ((uintptr_t)f->bits & 15) return fail(SRX_ERR_INVALID, "%s: filter rows must be 16-byte aligned", who);
    if (f->n_filters < 1) return fail(SRX_ERR_INVALID, "%s: n_filters must be >= 1", who);
    return SRX_OK;
}

int srx_check_row_builder(const char *who, const char *ids, int32_t n_rows, const int32_t *all_ptr, const int32_t *all_ids,
                          const int32_t *any_ptr, const int32_t *any_ids, const int32_t *none_ptr, const int32_t *none_ids,
                          const uint32_t *out_bits, const srx_doc_filter *base) {
    if (n_rows < 0) return fail(SRX_ERR_INVALID, "%s: n_rows < 0", who);
    if (!all_ptr != !all_ids || !any_ptr != !any_ids || !none_ptr != !none_ids) {
        snprintf(g_err, sizeof(g_err), "%s: the ptr and %s arrays of a list go together (both or neither)", who, ids);
        return SRX_ERR_INVALID;
    }
    if (!out_bits) return fail(SRX_ERR_INVALID, "%s: null out_bits", who);
    if ((uintptr_t)out_bits & 15) return fail(SRX_ERR_INVALID, "%s: filter rows must be 16-byte aligned", who);
    return base ? srx_check_filter(who, base) : SRX_OK;
}

int srx_launch_filtered_topk(const float *scores, int64_t ld, int64_t n_docs, int nq, int k, int n_splits, int64_t doc_base,
                             const srx_doc_filter &filter, int q0, const srx_rows &cand, hipStream_t stream) {
    hipLaunchKernelGGL(srx_filtered_topk_kernel, dim3((unsigned)((int64_t)nq * n_splits)), dim3(THREADS), 0, stream, scores, ld, n_docs, nq, k,
                       n_splits, doc_base, filter.bits, srx_filter_row_words(n_docs), filter.q_filter, q0, cand.doc, cand.score, cand.count);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int64_t srx_filter_words(int64_t n_docs) {
    if (n_docs < 1 || n_docs > SRX_FILTER_MAX_DOCS) return fail(SRX_ERR_INVALID, "srx_filter_words: n_docs must be in [1, 2^31 - 2]%s");
    return srx_filter_row_words(n_docs);
}

SRX_API int srx_filter_fill(int32_t device, uint32_t *bits, int32_t n_filters, int64_t n_docs, int32_t value, void *stream_v) {
    const int rc = check_rows("srx_filter_fill", bits, n_docs);
    if (rc != SRX_OK) return rc;
    if (n_filters < 1) return fail(SRX_ERR_INVALID, "srx_filter_fill: n_filters must be >= 1%s");
    if (value != 0 && value != 1) return fail(SRX_ERR_INVALID, "srx_filter_fill: value must be 0 or 1%s");
    HIP_TRY(hipSetDevice(device));
    const int64_t words = srx_filter_row_words(n_docs), total = words * n_filters;
    hipLaunchKernelGGL(srx_filter_fill_kernel, dim3(grid_for(total)), dim3(THREADS), 0, (hipStream_t)stream_v, bits, total, words, n_docs,
                       (int)value);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int srx_filter_set_docs(int32_t device, uint32_t *row_bits, int64_t n_docs, int64_t doc_base, const int32_t *doc, int64_t n,
                                int32_t value, void *stream_v) {
    const int rc = check_rows("srx_filter_set_docs", row_bits, n_docs);
    if (rc != SRX_OK) return rc;
    if (doc_base < 0 || doc_base + n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "srx_filter_set_docs: doc_base + n_docs must fit int32%s");
    if (value != 0 && value != 1) return fail(SRX_ERR_INVALID, "srx_filter_set_docs: value must be 0 or 1%s");
    if (n < 0) return fail(SRX_ERR_INVALID, "srx_filter_set_docs: n < 0%s");
    if (n == 0) return SRX_OK;
    if (!doc) return fail(SRX_ERR_INVALID, "srx_filter_set_docs: null pointer%s");
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(srx_filter_set_docs_kernel, dim3(grid_for(n)), dim3(THREADS), 0, (hipStream_t)stream_v, row_bits, n_docs, doc_base,
                       doc, n, (int)value);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int srx_filter_count(int32_t device, const uint32_t *bits, int32_t n_filters, int64_t n_docs, int32_t *out_count, void *stream_v) {
    const int rc = check_rows("srx_filter_count", bits, n_docs);
    if (rc != SRX_OK) return rc;
    if (n_filters < 1) return fail(SRX_ERR_INVALID, "srx_filter_count: n_filters must be >= 1%s");
    if (!out_count) return fail(SRX_ERR_INVALID, "srx_filter_count: null pointer%s");
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(srx_filter_count_kernel, dim3((unsigned)n_filters), dim3(THREADS), 0, (hipStream_t)stream_v, bits,
                       srx_filter_row_words(n_docs), n_docs, out_count);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
