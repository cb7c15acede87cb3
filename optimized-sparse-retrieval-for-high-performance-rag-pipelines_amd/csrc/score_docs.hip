// score_docs.hip -- exact sparse scores of caller-given candidate docs (srx_score_docs): "what does THIS doc score for
// this query?", the question none of the searches answers.  Same build flags as the other units; -ffp-contract=off is the
// contract here: a contribution is two fp32 multiplies, (v * idf) * qw, and a score the fp32 sum of the contributions in
// the order the query lists its terms -- the arithmetic of srx_search, so a row of srx_search scores to its own bits.
//
// One lane per (query, candidate) pair p = q * m + c.  Per query term the lane walks a short DEPENDENT load chain through
// the blocked layout (include/sparse_rx.h, srx_index_desc):
//     t = q_term[i]  ->  term_ptr[t], tile_skip[t][j], tile_skip[t][j + 1], idf[t]     (j = the doc's tile; 4 loads side by side)
//                    ->  lower-bound search for the doc in [term_ptr + skip[j], term_ptr + skip[j + 1])   (<= tile_log2 + 1 probes)
//                    ->  the posting's id and value (adjacent: one block)
// Ids are compared UNSIGNED: canonical sentinels are negative and compact ones are local ids >= 49152, so both sort behind
// every real id of the range (a unit's padding sits at the end of the unit's last tile) and the range is ascending as it
// stands -- no sentinel test.  In the compact copy the key is doc - first doc of its unit.
// The kernel is latency-bound (one HBM miss ~900 cycles, a chain of 5-18 loads), so the levers are independent chains in
// flight: SD_CHAINS consecutive terms of a pair are searched in lock step, branch-free -- an exhausted chain re-reads its
// final position, which is always inside the array: every position <= term_ptr[vocab] is followed by SRX_BLOCK_PAD
// sentinel blocks -- their contributions are kept in registers and added in term order.  No LDS, no atomics, no
// cross-lane operation: any (nq, m) is the same code.
#include "desc_check.h"

namespace {

constexpr int SD_CHAINS = 4;  // terms of one pair searched side by side

struct ScoreDocsArgs {
    const int64_t *term_ptr;
    const int32_t *post;  // the copy the instance reads: canonical blocks, or the compact copy
    const int32_t *tile_skip;
    const float *idf;
    const int32_t *q_ptr, *q_term;
    const float *q_weight;
    const int32_t *cand_doc, *cand_count;
    float *out_score;
    int64_t n_docs, doc_base;
    unsigned total;  // nq * m
    int m, tile_log2, n_tiles, unit_tiles;
};

__device__ __forceinline__ unsigned gload_u16(const void *p) { return *(const SRX_GLOBAL unsigned short *)p; }
__device__ __forceinline__ float gload_f32(const float *p) { return *(const SRX_GLOBAL float *)p; }
__device__ __forceinline__ int64_t gload_i64(const int64_t *p) { return *(const SRX_GLOBAL int64_t *)p; }

// Posting r (a padded position relative to the term's first block `blk`; term_ptr is a multiple of 4, so the block of
// position term_ptr + r is blk + (r >> 2) and its slot r & 3): the id as the search key compares it, and the value.
template <typename VT, bool COMPACT>
__device__ __forceinline__ unsigned sd_key_at(const int32_t *blk, unsigned r) {
    if constexpr (COMPACT)
        return gload_u16(reinterpret_cast<const unsigned short *>(blk + (size_t)(r >> 2) * CompactWords<VT>::value) + (r & 3u));
    else
        return (unsigned)gload_i32(blk + (size_t)(r >> 2) * BlockWords<VT>::value + (r & 3u));
}
template <typename VT, bool COMPACT>
__device__ __forceinline__ float sd_val_at(const int32_t *blk, unsigned r) {
    constexpr int W = COMPACT ? CompactWords<VT>::value : BlockWords<VT>::value;
    constexpr int V0 = COMPACT ? 2 : 4;  // first value word of a block
    const int32_t *v = blk + (size_t)(r >> 2) * W + V0;
    if constexpr (sizeof(VT) == 4)
        return __int_as_float(gload_i32(v + (r & 3u)));
    else
        return __half2float(__ushort_as_half((unsigned short)gload_u16(reinterpret_cast<const unsigned short *>(v) + (r & 3u))));
}

// 8 waves per SIMD (64 VGPRs): a 1024 x 100 batch is 1600 waves, less than one round of the chip's 8192 wave slots.
template <typename VT, bool COMPACT>
__global__ __launch_bounds__(THREADS, 8) void srx_score_docs_kernel(ScoreDocsArgs a) {
    const unsigned p = blockIdx.x * (unsigned)THREADS + threadIdx.x;
    if (p >= a.total) return;
    const unsigned q = p / (unsigned)a.m, c = p - q * (unsigned)a.m;
    bool live = true;
    if (a.cand_count != nullptr) live = (int)c < max(gload_i32(a.cand_count + q), 0);
    const int64_t local = (int64_t)gload_i32(a.cand_doc + p) - a.doc_base;
    live = live && local >= 0 && local < a.n_docs;
    int i = 0, iend = 0;
    if (live) {
        i = gload_i32(a.q_ptr + q);
        iend = gload_i32(a.q_ptr + q + 1);
    }
    const int j = live ? (int)(local >> a.tile_log2) : 0;  // the doc's tile, < n_tiles
    unsigned key = (unsigned)local;
    if constexpr (COMPACT) key = (unsigned)(local - (int64_t)(j / a.unit_tiles) * ((int64_t)a.unit_tiles << a.tile_log2));
    const int64_t row = (int64_t)a.n_tiles + 1;
    float s = 0.0f;
    for (; i < iend; i += SD_CHAINS) {
        const int32_t *blk[SD_CHAINS];
        unsigned lo[SD_CHAINS], hi[SD_CHAINS], end[SD_CHAINS];
        float w[SD_CHAINS];  // idf, then the contribution
        bool on[SD_CHAINS];
        int t[SD_CHAINS];
#pragma unroll
        for (int n = 0; n < SD_CHAINS; ++n) {
            on[n] = i + n < iend;
            t[n] = gload_i32(a.q_term + min(i + n, iend - 1));  // a chain past the query's end repeats the last term ...
        }
#pragma unroll
        for (int n = 0; n < SD_CHAINS; ++n) {
            // ... and searches the empty range [0, 0) of its first block: no branch around any load
            const int32_t *sk = a.tile_skip + (int64_t)t[n] * row + j;
            const unsigned s0 = (unsigned)gload_i32(sk), s1 = (unsigned)gload_i32(sk + 1);
            lo[n] = on[n] ? s0 : 0u;
            end[n] = on[n] ? s1 : 0u;
            hi[n] = end[n];
            constexpr int W = COMPACT ? CompactWords<VT>::value : BlockWords<VT>::value;
            blk[n] = a.post + (gload_i64(a.term_ptr + t[n]) >> 2) * W;
            w[n] = gload_f32(a.idf + t[n]);
        }
        for (;;) {  // lower bound of `key` in every chain's range, one probe per chain and round
            bool any = false;
#pragma unroll
            for (int n = 0; n < SD_CHAINS; ++n) any = any || lo[n] < hi[n];
            if (!any) break;
            unsigned mid[SD_CHAINS], d[SD_CHAINS];
#pragma unroll
            for (int n = 0; n < SD_CHAINS; ++n) {
                mid[n] = lo[n] + ((hi[n] - lo[n]) >> 1);
                d[n] = sd_key_at<VT, COMPACT>(blk[n], mid[n]);
            }
#pragma unroll
            for (int n = 0; n < SD_CHAINS; ++n) {
                const bool open = lo[n] < hi[n], right = d[n] < key;
                lo[n] = (open && right) ? mid[n] + 1u : lo[n];
                hi[n] = (open && !right) ? mid[n] : hi[n];
            }
        }
        float v[SD_CHAINS];
        unsigned d[SD_CHAINS];
#pragma unroll
        for (int n = 0; n < SD_CHAINS; ++n) {
            d[n] = sd_key_at<VT, COMPACT>(blk[n], lo[n]);
            v[n] = sd_val_at<VT, COMPACT>(blk[n], lo[n]);
        }
#pragma unroll
        for (int n = 0; n < SD_CHAINS; ++n) {
            const bool hit = lo[n] < end[n] && d[n] == key;
            const float qw = gload_f32(a.q_weight + min(i + n, iend - 1));
            w[n] = (v[n] * w[n]) * qw;
            if (hit) s = s + w[n];  // in term order
        }
    }
    a.out_score[p] = s;
}

template <typename VT, bool COMPACT>
int launch_score_docs(const ScoreDocsArgs &a, hipStream_t stream) {
    const unsigned blocks = (a.total + THREADS - 1) / THREADS;
    hipLaunchKernelGGL((srx_score_docs_kernel<VT, COMPACT>), dim3(blocks), dim3(THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

}  // namespace

int srx_check_index_desc(const char *who, const srx_index_desc *d) {
    if (!d) return fail(SRX_ERR_INVALID, "%s: null descriptor", who);
    if (d->val_type != SRX_VAL_F32 && d->val_type != SRX_VAL_F16) return fail(SRX_ERR_INVALID, "%s: bad val_type", who);
    if (d->n_docs <= 0 || d->n_docs >= 0x7FFFFFFFll || d->vocab <= 0) return fail(SRX_ERR_INVALID, "%s: n_docs / vocab out of range", who);
    if (d->tile_log2 < 6 || d->tile_log2 > SRX_MAX_TILE_LOG2) return fail(SRX_ERR_INVALID, "%s: tile_log2 must be in [6, 14]", who);
    if ((int64_t)d->n_tiles != (d->n_docs + (1ll << d->tile_log2) - 1) >> d->tile_log2)
        return fail(SRX_ERR_INVALID, "%s: n_tiles != ceil(n_docs / 2^tile_log2)", who);
    if (d->unit_tiles < 1 || d->unit_tiles > MAX_TPS) return fail(SRX_ERR_INVALID, "%s: unit_tiles must be in [1, 64]", who);
    if (!d->post && !d->post16) return fail(SRX_ERR_INVALID, "%s: the descriptor has neither post nor post16", who);
    if (d->post16 && ((int64_t)d->unit_tiles << d->tile_log2) > W_UNIT_MAX_DOCS)
        return fail(SRX_ERR_INVALID, "%s: a compact copy (post16) needs units of <= 49152 docs", who);
    if (!d->term_ptr || !d->tile_skip || !d->idf) return fail(SRX_ERR_INVALID, "%s: null term_ptr / tile_skip / idf", who);
    return SRX_OK;
}

SRX_API int srx_score_docs(const srx_index_desc *d, const int32_t *q_ptr, const int32_t *q_term, const float *q_weight,
                           int32_t nq, const int32_t *cand_doc, const int32_t *cand_count, int32_t m, float *out_score,
                           void *stream_v) {
    const int rc = srx_check_index_desc("srx_score_docs", d);
    if (rc != SRX_OK) return rc;
    if (nq < 0) return fail(SRX_ERR_INVALID, "srx_score_docs: nq < 0%s");
    if (m < 1) return fail(SRX_ERR_INVALID, "srx_score_docs: m must be >= 1%s");
    if ((int64_t)nq * (int64_t)m > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "srx_score_docs: nq * m must fit int32%s");
    if (nq == 0) return SRX_OK;
    if (!q_ptr || !cand_doc || !out_score) return fail(SRX_ERR_INVALID, "srx_score_docs: null q_ptr / cand_doc / out_score%s");
    HIP_TRY(hipSetDevice(d->device));
    hipStream_t stream = (hipStream_t)stream_v;
    const bool compact = d->post16 != nullptr;
    const ScoreDocsArgs a = {d->term_ptr, compact ? d->post16 : d->post, d->tile_skip, d->idf, q_ptr, q_term, q_weight,
                             cand_doc, cand_count, out_score, d->n_docs, d->doc_base, (unsigned)((int64_t)nq * m), m,
                             d->tile_log2, d->n_tiles, d->unit_tiles};
    if (d->val_type == SRX_VAL_F32)
        return compact ? launch_score_docs<float, true>(a, stream) : launch_score_docs<float, false>(a, stream);
    return compact ? launch_score_docs<__half, true>(a, stream) : launch_score_docs<__half, false>(a, stream);
}
