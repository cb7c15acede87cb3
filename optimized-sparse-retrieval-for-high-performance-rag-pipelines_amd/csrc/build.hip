// build.hip -- index-build kernels and the srx_build_* entry points of the C ABI: BM25 impacts, the tile skip table, the
// blocked posting layout (padded runs of [4 docs | 4 values] blocks, srx_common.h) with its compact copy, the per-term score
// bounds and the sums of duplicate COO entries.  None of it runs during a search.

#include "srx_common.h"

namespace {

__global__ void srx_impact_kernel(const float *__restrict__ tf, const int32_t *__restrict__ post_doc,
                                  const float *__restrict__ doc_len, int64_t nnz, float k1f, float bf, float omb,
                                  float k1p1, float avf, float *__restrict__ out) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
        const float t = tf[p];
        const float len = doc_len[post_doc[p]];
        const float norm = k1f * (omb + (bf * len) / avf);  // retrieval.py:58
        out[p] = (t * k1p1) / (t + norm);                   // retrieval.py:70-72
    }
}

__global__ void srx_tile_skip_kernel(const int64_t *__restrict__ term_ptr, const int32_t *__restrict__ post_doc,
                                     int64_t vocab, int n_tiles, int tile_log2, int32_t *__restrict__ out) {
    const int64_t total = vocab * (int64_t)(n_tiles + 1);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = e / (n_tiles + 1);
        const int j = (int)(e - t * (n_tiles + 1));
        const int64_t b = term_ptr[t], en = term_ptr[t + 1];
        const int64_t target = (int64_t)j << tile_log2;
        int64_t lo = b, hi = en;  // lower_bound(post_doc[b..en), target)
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if ((int64_t)post_doc[mid] < target)
                lo = mid + 1;
            else
                hi = mid;
        }
        out[e] = (int32_t)(lo - b);
    }
}

// ---- layout v2: scatter the term-major postings into padded runs of blocks (srx_common.h, IndexView) ----
// skip   = the UNPADDED tile skip table (srx_tile_skip_kernel on the plain CSC arrays)
// runpad = [vocab * n_units + 1] exclusive prefix of the PADDED run lengths (padded position of every run's start)
// One thread per posting: its run, its rank inside the run, its slot in the blocks; the thread of a run's last posting
// also writes the run's sentinels (doc -1, value 0).
template <typename VT>
__global__ void srx_blocks_scatter_kernel(const int64_t *__restrict__ term_ptr, const int32_t *__restrict__ post_term,
                                          const int32_t *__restrict__ post_doc, const VT *__restrict__ post_val,
                                          const int32_t *__restrict__ skip, const int64_t *__restrict__ runpad, int64_t nnz,
                                          int n_tiles, int tile_log2, int unit_tiles, int n_units,
                                          int32_t *__restrict__ out_post) {
    constexpr int BW = BlockWords<VT>::value;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < nnz; p += (int64_t)gridDim.x * blockDim.x) {
        const int t = post_term[p];
        const int doc = post_doc[p];
        const int u = (doc >> tile_log2) / unit_tiles;
        const int32_t *row = skip + (int64_t)t * (n_tiles + 1);
        const int ja = u * unit_tiles, jb = min(ja + unit_tiles, n_tiles);
        const int64_t i = p - term_ptr[t];               // rank inside the term
        const int64_t kr = i - row[ja];                   // rank inside the run
        int64_t dst = runpad[(int64_t)t * n_units + u] + kr;
        auto put = [&](int64_t q, int d, VT v) {
            int32_t *blk = out_post + (q >> 2) * BW;
            blk[q & 3] = d;
            reinterpret_cast<VT *>(blk + 4)[q & 3] = v;
        };
        put(dst, doc, post_val[p]);
        if (i + 1 == row[jb]) {                           // last posting of its run: pad to a multiple of 4
            // sentinel doc ids -1 - 32 * (t % 64): value 0 makes them no-ops; different terms' sentinels fall into
            // different words of the tier-1 bitmap (an LDS atomic of several lanes on ONE address serialises)
            for (++dst; (dst & 3) != 0; ++dst) put(dst, -1 - 32 * (t & 63), VT(0.0f));
        }
    }
}

// padded tile skip table + padded term offsets from the unpadded table and the run prefix
__global__ void srx_blocks_skip_kernel(const int32_t *__restrict__ skip, const int64_t *__restrict__ runpad, int64_t vocab,
                                       int n_tiles, int unit_tiles, int n_units, int32_t *__restrict__ out_skip,
                                       int64_t *__restrict__ out_term_ptr) {
    const int64_t total = vocab * (int64_t)(n_tiles + 1);
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t t = e / (n_tiles + 1);
        const int j = (int)(e - t * (n_tiles + 1));
        const int64_t r0 = runpad[t * n_units];
        if (j == n_tiles) {
            out_skip[e] = (int32_t)(runpad[(t + 1) * n_units] - r0);  // all of the term, padding included
        } else {
            const int u = j / unit_tiles;
            out_skip[e] = (int32_t)(runpad[t * n_units + u] - r0) + (skip[e] - skip[t * (n_tiles + 1) + u * unit_tiles]);
        }
        if (j == 0) out_term_ptr[t] = r0;
        if (e == total - 1) out_term_ptr[vocab] = runpad[vocab * n_units];
    }
}

template <typename VT>
__global__ void srx_blocks_sentinel_kernel(int32_t *__restrict__ out_post, int64_t first_block, int n) {
    constexpr int BW = BlockWords<VT>::value;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // posting slot
    if (i < 4 * n) {
        int32_t *blk = out_post + (first_block + (i >> 2)) * BW;
        blk[i & 3] = -1 - 32 * ((i >> 2) & 63);  // block j: doc -1 - 32 (j mod 64) -> bitmap word 2047 - j mod 64: the idle loads of one
                                                // step (blocks lane + const) hit a word of their own per lane
        reinterpret_cast<VT *>(blk + 4)[i & 3] = VT(0.0f);
    }
}

// Compact copy for tier 1 (srx_common.h, CompactWords): one thread per block, 16-bit unit-local doc ids.
template <typename VT>
__global__ void srx_compact_blocks_kernel(const int32_t *__restrict__ post, int64_t n_blocks_total, int unit_docs,
                                          int32_t *__restrict__ out) {
    constexpr int BW = BlockWords<VT>::value, CW = CompactWords<VT>::value;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks_total) return;
    const int32_t *src = post + b * BW;
    int32_t *dst = out + b * CW;
    unsigned l[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int d = src[c];
        l[c] = d >= 0 ? (unsigned)(d % unit_docs) : (unsigned)W_SENT_BASE + 32u * (unsigned)(((-1 - d) >> 5) & 63);
    }
    dst[0] = (int32_t)(l[0] | (l[1] << 16));
    dst[1] = (int32_t)(l[2] | (l[3] << 16));
#pragma unroll
    for (int c = 4; c < BW; ++c) dst[c - 2] = src[c];  // the values, unchanged
}

// ------------------------------------------------------------------------------------------------
// Term bounds: out[t * nk + j] = the ks[j]-th largest stored value of term t (0 when it has fewer than ks[j] positive
// values).  One workgroup per term (grid-stride): the term's run of the term-major value array is folded into the
// exact lazy top-k list of the search kernels (k = the largest rank asked for, <= 1 024), then every kept value counts
// the kept values above it and equal to it and writes the ranks it covers.  One streaming pass over the values; the
// first form was a 64-bit sort of (term, value) keys of ALL postings (16+ bytes of temporary memory per posting, the
// build's peak).  A negative value raises *neg_flag (the bounds are only valid for non-negative values).
constexpr int TB_NPT = 16;
template <typename VT>
__global__ __launch_bounds__(THREADS) void srx_term_bounds_kernel(const int64_t *__restrict__ term_ptr, const VT *__restrict__ val,
                                                                  int64_t vocab, const int32_t *__restrict__ ks, int nk, int kmax,
                                                                  float *__restrict__ out, int *__restrict__ neg_flag) {
    __shared__ MergeShared M;
    const int tid = threadIdx.x;
    for (int64_t t = blockIdx.x; t < vocab; t += gridDim.x) {
        const int64_t lo = term_ptr[t], hi = term_ptr[t + 1];
        if (tid < nk) out[t * nk + tid] = 0.0f;
        if (tid == 0) {
            M.tk.count = 0;
            M.tk.tau = 0;
        }
        __syncthreads();
        bool neg = false;
        for (int64_t c0 = lo; c0 < hi; c0 += (int64_t)THREADS * TB_NPT) {
            unsigned ubits[TB_NPT];
            int udoc[TB_NPT];
            const unsigned tau = M.tk.tau;
#pragma unroll
            for (int n = 0; n < TB_NPT; ++n) {
                const int64_t c = c0 + (int64_t)n * THREADS + tid;
                float x = 0.0f;
                if (c < hi) x = (float)val[c];
                neg |= x < 0.0f;
                const unsigned b = __float_as_uint(x);
                ubits[n] = (x > 0.0f && b >= tau) ? b : 0u;
                udoc[n] = (int)(c - lo);
            }
            topk_fold<TB_NPT, true>(ubits, udoc, kmax, M.tk, M.hist);
        }
        if (neg) *neg_flag = 1;
        __syncthreads();
        topk_shrink(kmax, M.tk, M.hist);
        __syncthreads();
        const unsigned cnt = M.tk.count;
        for (unsigned i = tid; i < cnt; i += THREADS) {
            const unsigned xi = M.tk.bits[i];
            int gt = 0, eq = 0;
            for (unsigned j = 0; j < cnt; ++j) {  // every thread reads the same word: an LDS broadcast
                const unsigned xj = M.tk.bits[j];
                gt += xj > xi;
                eq += xj == xi;
            }
            for (int j = 0; j < nk; ++j) {
                const int K = ks[j];
                if (gt < K && K <= gt + eq) out[t * nk + j] = __uint_as_float(xi);  // ties write the same value
            }
        }
        __syncthreads();  // the list is re-initialised by the next term
    }
}

// Duplicate (doc, term) entries of a COO input, adjacent after the stable term sort: group g = entries
// [first[g], first[g + 1]) is summed left to right in input order, like SciPy sums duplicates when the reference assembles
// its CSR (csr_matrix((data, (rows, cols))), retrieval.py:171-175).  One thread per group (groups are almost all of length 1).
__global__ __launch_bounds__(256) void srx_sum_groups_kernel(const int64_t *__restrict__ first, int64_t n_groups,
                                                             const float *__restrict__ val, float *__restrict__ out) {
    for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n_groups; g += (int64_t)gridDim.x * 256) {
        const int64_t a = first[g], b = first[g + 1];
        float s = val[a];
        for (int64_t i = a + 1; i < b; ++i) s = s + val[i];
        out[g] = s;
    }
}
}  // namespace

SRX_API int srx_build_impacts(int32_t device, const float *tf, const int32_t *post_doc, const float *doc_len,
                              int64_t nnz, double k1, double b, double avgdl, float *out_impact, void *stream_v) {
    if (nnz < 0 || (nnz > 0 && (!tf || !post_doc || !doc_len || !out_impact)))
        return fail(SRX_ERR_INVALID, "srx_build_impacts: bad argument%s");
    if (nnz == 0) return SRX_OK;
    HIP_TRY(hipSetDevice(device));
    int64_t blocks = (nnz + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(srx_impact_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_v, tf, post_doc, doc_len,
                       nnz, (float)k1, (float)b, (float)(1.0 - b), (float)(k1 + 1.0), (float)avgdl, out_impact);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int srx_build_sum_duplicates(int32_t device, const int64_t *first, int64_t n_groups, const float *val, float *out_sum,
                                     void *stream_v) {
    if (n_groups < 0 || (n_groups > 0 && (!first || !val || !out_sum))) return fail(SRX_ERR_INVALID, "srx_build_sum_duplicates: bad argument%s");
    if (n_groups == 0) return SRX_OK;
    HIP_TRY(hipSetDevice(device));
    int64_t blocks = (n_groups + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(srx_sum_groups_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_v, first, n_groups, val, out_sum);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int srx_build_tile_skip(int32_t device, const int64_t *term_ptr, const int32_t *post_doc, int64_t vocab,
                                int32_t n_tiles, int32_t tile_log2, int32_t *out_skip, void *stream_v) {
    if (!term_ptr || !out_skip || vocab <= 0 || n_tiles <= 0 || tile_log2 < 0 || tile_log2 > 30)
        return fail(SRX_ERR_INVALID, "srx_build_tile_skip: bad argument%s");
    HIP_TRY(hipSetDevice(device));
    const int64_t total = vocab * (int64_t)(n_tiles + 1);
    int64_t blocks = (total + 255) / 256;
    if (blocks > 16384) blocks = 16384;
    hipLaunchKernelGGL(srx_tile_skip_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream_v, term_ptr, post_doc,
                       vocab, n_tiles, tile_log2, out_skip);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int32_t srx_auto_unit_tiles(int64_t n_docs, int64_t vocab, int64_t nnz, int32_t tile_log2) {
    if (n_docs <= 0 || vocab <= 0 || nnz < 0 || tile_log2 < 6 || tile_log2 > SRX_MAX_TILE_LOG2)
        return fail(SRX_ERR_INVALID, "srx_auto_unit_tiles: bad argument%s");
    // The largest unit (in tiles) for which the run of an average term inside a unit overflows the registers of its lane
    // group (8 lanes x W_R postings in the reference case of an 8-term query) with negligible probability (mean +
    // 5 sigma, Poisson), and whose docs fit the tier-1 bitmap / the compact copy's local ids (49152).
    const int max_tpu_bitmap = W_UNIT_MAX_DOCS >> tile_log2;  // 16-bit unit-local ids below the sentinels' range (>= 3 tiles of 16384)
    const double per_doc_per_term = (double)nnz / ((double)n_docs * (double)vocab);
    auto fits = [&](int t) {
        const double mean = per_doc_per_term * (double)t * (double)(1ll << tile_log2);
        return mean + 5.0 * sqrt(mean) <= 8.0 * W_R;
    };
    int tpu = 1;
    while (tpu < MAX_TPS && tpu < max_tpu_bitmap && fits(tpu + 1)) ++tpu;
    return tpu;
}

SRX_API int srx_build_compact(int32_t device, int32_t val_type, const int32_t *post, int64_t n_blocks_total, int32_t tile_log2,
                              int32_t unit_tiles, int32_t *out_post16, void *stream_v) {
    if (!post || !out_post16 || n_blocks_total <= 0) return fail(SRX_ERR_INVALID, "srx_build_compact: bad argument%s");
    if (val_type != SRX_VAL_F32 && val_type != SRX_VAL_F16) return fail(SRX_ERR_INVALID, "srx_build_compact: bad val_type%s");
    if (tile_log2 < 6 || tile_log2 > SRX_MAX_TILE_LOG2 || unit_tiles < 1 || ((int64_t)unit_tiles << tile_log2) > W_UNIT_MAX_DOCS)
        return fail(SRX_ERR_INVALID, "srx_build_compact: a unit must cover at most 49152 docs (the tier-1 bitmap; the sentinels' local ids lie above)%s");
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    const unsigned grid = (unsigned)((n_blocks_total + 255) / 256);
    const int unit_docs = unit_tiles << tile_log2;
    if (val_type == SRX_VAL_F32)
        hipLaunchKernelGGL(srx_compact_blocks_kernel<float>, dim3(grid), dim3(256), 0, stream, post, n_blocks_total, unit_docs, out_post16);
    else
        hipLaunchKernelGGL(srx_compact_blocks_kernel<__half>, dim3(grid), dim3(256), 0, stream, post, n_blocks_total, unit_docs, out_post16);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int srx_build_blocks(int32_t device, int32_t val_type, const int64_t *term_ptr, const int32_t *post_term,
                             const int32_t *post_doc, const void *post_val, const int32_t *skip, const int64_t *runpad,
                             int64_t vocab, int64_t nnz, int32_t n_tiles, int32_t tile_log2, int32_t unit_tiles,
                             int32_t *out_post, int32_t *out_skip, int64_t *out_term_ptr, int64_t n_blocks, void *stream_v) {
    if (!term_ptr || !skip || !runpad || !out_post || !out_skip || !out_term_ptr || vocab <= 0 || nnz < 0 || n_tiles <= 0 ||
        unit_tiles < 1 || n_blocks < 0 || (nnz > 0 && (!post_term || !post_doc || !post_val)))
        return fail(SRX_ERR_INVALID, "srx_build_blocks: bad argument%s");
    if (val_type != SRX_VAL_F32 && val_type != SRX_VAL_F16) return fail(SRX_ERR_INVALID, "srx_build_blocks: bad val_type%s");
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    const int n_units = (n_tiles + unit_tiles - 1) / unit_tiles;
    if (nnz > 0) {
        int64_t blocks = (nnz + 255) / 256;
        if (blocks > 16384) blocks = 16384;
        if (val_type == SRX_VAL_F32)
            hipLaunchKernelGGL(srx_blocks_scatter_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, stream, term_ptr, post_term,
                               post_doc, (const float *)post_val, skip, runpad, nnz, n_tiles, tile_log2, unit_tiles, n_units, out_post);
        else
            hipLaunchKernelGGL(srx_blocks_scatter_kernel<__half>, dim3((unsigned)blocks), dim3(256), 0, stream, term_ptr, post_term,
                               post_doc, (const __half *)post_val, skip, runpad, nnz, n_tiles, tile_log2, unit_tiles, n_units, out_post);
        HIP_TRY(hipGetLastError());
    }
    {
        const int64_t total = vocab * (int64_t)(n_tiles + 1);
        int64_t blocks = (total + 255) / 256;
        if (blocks > 16384) blocks = 16384;
        hipLaunchKernelGGL(srx_blocks_skip_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, skip, runpad, vocab, n_tiles, unit_tiles,
                           n_units, out_skip, out_term_ptr);
        HIP_TRY(hipGetLastError());
    }
    // the SRX_BLOCK_PAD sentinel blocks behind the last run: lane j of a tier-1 wave redirects its idle loads to block n_blocks + j
    if (val_type == SRX_VAL_F32)
        hipLaunchKernelGGL(srx_blocks_sentinel_kernel<float>, dim3(SRX_BLOCK_PAD * 4 / 64), dim3(64), 0, stream, out_post, n_blocks, SRX_BLOCK_PAD);
    else
        hipLaunchKernelGGL(srx_blocks_sentinel_kernel<__half>, dim3(SRX_BLOCK_PAD * 4 / 64), dim3(64), 0, stream, out_post, n_blocks, SRX_BLOCK_PAD);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int srx_build_term_bounds(int32_t device, int32_t val_type, const int64_t *term_ptr, const void *post_val, int64_t vocab,
                                  const int32_t *ks, int32_t nk, float *out_bound, int32_t *neg_flag, void *stream_v) {
    if (!term_ptr || !post_val || !ks || !out_bound || !neg_flag || vocab <= 0 || nk <= 0 || nk > 64)
        return fail(SRX_ERR_INVALID, "srx_build_term_bounds: bad argument (1 <= nk <= 64)%s");
    if (val_type != SRX_VAL_F32 && val_type != SRX_VAL_F16) return fail(SRX_ERR_INVALID, "srx_build_term_bounds: unknown val_type%s");
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    int32_t hks[64];
    HIP_TRY(hipMemcpyAsync(hks, ks, sizeof(int32_t) * nk, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    int kmax = 0;
    for (int j = 0; j < nk; ++j) {
        if (hks[j] < 1 || hks[j] > KMAX) return fail(SRX_ERR_INVALID, "srx_build_term_bounds: ranks must be in 1 .. 1024%s");
        if (hks[j] > kmax) kmax = hks[j];
    }
    HIP_TRY(hipMemsetAsync(neg_flag, 0, sizeof(int32_t), stream));
    const unsigned blocks = (unsigned)(vocab < 256 * 16 ? vocab : 256 * 16);
    if (val_type == SRX_VAL_F32)
        hipLaunchKernelGGL(srx_term_bounds_kernel<float>, dim3(blocks), dim3(THREADS), 0, stream, term_ptr, (const float *)post_val, vocab,
                           ks, (int)nk, kmax, out_bound, (int *)neg_flag);
    else
        hipLaunchKernelGGL(srx_term_bounds_kernel<__half>, dim3(blocks), dim3(THREADS), 0, stream, term_ptr, (const __half *)post_val,
                           vocab, ks, (int)nk, kmax, out_bound, (int *)neg_flag);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
