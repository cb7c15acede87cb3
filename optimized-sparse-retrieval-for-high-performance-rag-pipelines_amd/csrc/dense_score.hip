// dense_score.hip -- dense scores of caller-given candidate docs (srx_dense_score_docs_f32 / _u8 / _i8,
// include/sparse_rx_rescore.h): the dense twins of srx_score_docs.  Same build flags as the other units;
// -ffp-contract=off is the contract of the f32 / u8 forms: the arithmetic is that of the search kernels in dense.hip
// (srx_dense_f32_scores_kernel, srx_dense_u8_scores_kernel, srx_dense_i8_scores_kernel), so a row a dense search
// returned scores to its own bits.
//
// One wave per (query, chunk of DS_CHUNK = 64 of that query's candidates).  Lane j reads candidate j's id once and decides
// whether it is live (inside cand_count, inside the corpus); the ids then travel by lane permute.  The query sits in
// registers once per wave.  The work is a gather of 64 B .. 4 KiB rows -- latency, not bandwidth -- so U candidate rows are
// loaded before the first is used; groups of U without a live candidate are skipped, and a dead candidate's loads are
// masked off (no corpus byte is read for it).
//   f32 / u8   the lane layout is the search's: lane l holds columns l, l + 64, ... of the row; products summed in
//              ascending slice order, then the fixed xor butterfly.  NS (slices held) is a compile-time bucket >= dim / 64:
//              the slices beyond dim are zeros on both sides and change no bit.
//   i8         a row is dim / 16 pieces of 16 bytes; G = the next power of two lanes share a candidate (lane sub < dim / 16
//              holds piece sub of the query and of the row), 64 / G candidates per load round.  The int32 dot product is
//              exact in any order; the fp64 scaling is the search's expression.
// No LDS, no atomics, no workspace.
#include "srx_common.h"
#include "sparse_rx_rescore.h"

namespace {

typedef int ds_v4i __attribute__((ext_vector_type(4)));
constexpr int DS_CHUNK = 64;  // candidates per wave: one per lane

struct DenseScoreArgs {
    const void *corpus;        // f32 / u8 / i8 rows (i8: row-major or fragment order)
    const float *corpus_scale; // u8: f32[2 n_docs] (scale, min per doc); i8: f32[n_docs]
    const void *queries;       // f32[nq][dim] or i8[nq][dim]
    const float *query_scale;  // i8 only
    const int32_t *cand_doc, *cand_count;
    float *out_score;
    int64_t n_docs, doc_base, waves;  // waves = nq * chunks
    int dim, m, chunks;               // chunks of DS_CHUNK candidates per query
    int packed, glog;                 // i8: storage form; log2 of the lanes that share a candidate
};

// The wave's (query, chunk) and lane `lane`'s candidate: its row in the corpus, or -1 (padding, outside the corpus,
// beyond m).  False: the wave lies past the batch.
__device__ __forceinline__ bool ds_candidate(const DenseScoreArgs &a, int lane, int &q, int &c, int &row) {
    const int64_t w = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w >= a.waves) return false;  // whole waves leave
    q = (int)(w / a.chunks);
    c = (int)(w - (int64_t)q * a.chunks) * DS_CHUNK + lane;
    int lim = a.m;
    if (a.cand_count != nullptr) lim = min(lim, max(gload_i32(a.cand_count + q), 0));
    row = -1;
    if (c < lim) {
        const int64_t local = (int64_t)gload_i32(a.cand_doc + (int64_t)q * a.m + c) - a.doc_base;
        if (local >= 0 && local < a.n_docs) row = (int)local;  // n_docs < 2^31
    }
    return true;
}
// bits [lo, lo + n) of the live mask
__device__ __forceinline__ unsigned long long ds_mask_range(unsigned long long m, int lo, int n) {
    m >>= lo;
    return n >= 64 ? m : m & ((1ull << n) - 1ull);
}

template <int NS, int U, bool IS_U8>
__global__ __launch_bounds__(THREADS) void srx_dense_score_rows_kernel(DenseScoreArgs a) {
    const int lane = threadIdx.x & 63;
    int q, c, row;
    if (!ds_candidate(a, lane, q, c, row)) return;
    const unsigned long long live = __ballot(row >= 0);
    float res = 0.0f;  // candidate `lane`'s score
    if (live != 0ull) {  // uniform
        const int ns = a.dim >> 6;
        const float *qrow = (const float *)a.queries + (int64_t)q * a.dim;
        float qv[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) qv[i] = i < ns ? qrow[lane + 64 * i] : 0.0f;
        for (int c0 = 0; c0 < DS_CHUNK; c0 += U) {
            if (ds_mask_range(live, c0, U) == 0ull) continue;  // uniform
            float r[U][NS];
            int rw[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                rw[u] = __shfl(row, c0 + u);
                const bool on = rw[u] >= 0;
                if constexpr (IS_U8) {
                    const uint8_t *p = (const uint8_t *)a.corpus + (int64_t)rw[u] * a.dim;
                    float sc = 0.0f, mn = 0.0f;
                    if (on) {
                        sc = a.corpus_scale[2 * (int64_t)rw[u]];
                        mn = a.corpus_scale[2 * (int64_t)rw[u] + 1];
                    }
#pragma unroll
                    for (int i = 0; i < NS; ++i) r[u][i] = (on && i < ns) ? (float)p[lane + 64 * i] * sc + mn : 0.0f;
                } else {
                    const float *p = (const float *)a.corpus + (int64_t)rw[u] * a.dim;
#pragma unroll
                    for (int i = 0; i < NS; ++i) r[u][i] = (on && i < ns) ? p[lane + 64 * i] : 0.0f;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                float s = 0.0f;
#pragma unroll
                for (int i = 0; i < NS; ++i) s = s + r[u][i] * qv[i];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
                if (lane == c0 + u && rw[u] >= 0) res = s;  // every lane holds the same bits: the partners of a butterfly step add the same pair
            }
        }
    }
    if (c < a.m) a.out_score[(int64_t)q * a.m + c] = res;
}

__device__ __forceinline__ int ds_dot16(ds_v4i x, ds_v4i y) {
    int acc = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) acc = __builtin_amdgcn_sdot4(x[w], y[w], acc, false);
    return acc;
}

template <int U>
__global__ __launch_bounds__(THREADS) void srx_dense_score_i8_kernel(DenseScoreArgs a) {
    const int lane = threadIdx.x & 63;
    int q, c, row;
    if (!ds_candidate(a, lane, q, c, row)) return;
    if (row < 0 && c < a.m) a.out_score[(int64_t)q * a.m + c] = 0.0f;  // the dead candidates' words; the live ones' are written below
    const unsigned long long live = __ballot(row >= 0);
    if (live == 0ull) return;  // uniform
    const int pieces = a.dim >> 4, g = 1 << a.glog, per = 64 >> a.glog;  // candidates per load round
    const int sub = lane & (g - 1), slot = lane >> a.glog;
    const int8_t *corpus = (const int8_t *)a.corpus;
    ds_v4i qp = {0, 0, 0, 0};
    if (sub < pieces) qp = *reinterpret_cast<const ds_v4i *>((const int8_t *)a.queries + (int64_t)q * a.dim + 16 * sub);
    const double qs = (double)a.query_scale[q];
    const int ks = a.dim >> 5;
    for (int c0 = 0; c0 < DS_CHUNK; c0 += per * U) {
        if (ds_mask_range(live, c0, per * U) == 0ull) continue;  // uniform
        ds_v4i B[U];
        int rw[U];
        float cs[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int ci = c0 + u * per + slot;
            rw[u] = __shfl(row, ci);  // ci < DS_CHUNK: a round covers 64 >> glog candidates and U <= 1 << glog
            B[u] = (ds_v4i){0, 0, 0, 0};
            cs[u] = 0.0f;
            if (rw[u] >= 0) {
                const int64_t d = rw[u];
                cs[u] = a.corpus_scale[d];
                if (sub < pieces) {
                    const int64_t off = a.packed ? ((((d >> 5) * ks + (sub >> 1)) * 64 + (d & 31) + 32 * (sub & 1)) << 4) : d * a.dim + 16 * sub;
                    B[u] = *reinterpret_cast<const ds_v4i *>(corpus + off);
                }
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            int acc = ds_dot16(qp, B[u]);
            for (int o = g >> 1; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
            if (sub == 0 && rw[u] >= 0)  // live: inside the chunk and inside m
                a.out_score[(int64_t)q * a.m + (c - lane) + c0 + u * per + slot] = (float)(((double)acc * qs) * (double)cs[u]);
        }
    }
}

template <bool IS_U8>
void launch_rows(const DenseScoreArgs &a, unsigned blocks, hipStream_t stream) {
    const int ns = a.dim >> 6;
#define SRX_DS(NS, U)                                                                                                        \
    if (ns <= NS) {                                                                                                          \
        hipLaunchKernelGGL((srx_dense_score_rows_kernel<NS, U, IS_U8>), dim3(blocks), dim3(THREADS), 0, stream, a);          \
        return;                                                                                                              \
    }
    SRX_DS(1, 8) SRX_DS(2, 8) SRX_DS(4, 8) SRX_DS(8, 8) SRX_DS(16, 4)
#undef SRX_DS
}

// The checks the three forms share.  1 = nothing to do, 0 = go on, < 0 = refused
int ds_check(const char *who, int64_t n_docs, int32_t nq, int32_t m, const int32_t *cand_doc, const float *out_score) {
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if (m < 1) return fail(SRX_ERR_INVALID, "%s: m must be >= 1", who);
    if ((int64_t)nq * (int64_t)m > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: nq * m must fit int32", who);
    if (n_docs <= 0 || n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: n_docs out of range", who);
    if (nq == 0) return 1;
    if (!cand_doc || !out_score) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    return 0;
}

DenseScoreArgs ds_args(const void *corpus, const float *cscale, const void *queries, const float *qscale, int64_t n_docs, int32_t dim,
                       int32_t nq, int64_t doc_base, const int32_t *cand_doc, const int32_t *cand_count, int32_t m, float *out_score) {
    const int chunks = (m + DS_CHUNK - 1) / DS_CHUNK;
    return {corpus, cscale, queries, qscale, cand_doc, cand_count, out_score, n_docs, doc_base, (int64_t)nq * chunks, dim, m, chunks, 0, 0};
}
unsigned ds_blocks(const DenseScoreArgs &a) { return (unsigned)((a.waves + WAVES - 1) / WAVES); }  // waves <= nq * m < 2^31

// rows: f32 embeddings, or (is_u8) uint8 rows de-quantized with u8_scale_min
int dense_score_rows(const char *who, bool is_u8, int32_t device, const void *rows, const float *u8_scale_min, int64_t n_docs, int32_t dim,
                     const float *queries, int32_t nq, int64_t doc_base, const int32_t *cand_doc, const int32_t *cand_count,
                     int32_t m, float *out_score, void *stream_v) {
    if (dim <= 0 || dim % 64 != 0 || dim > 1024) return fail(SRX_ERR_INVALID, "%s: dim must be a multiple of 64, <= 1024 (pad the rows with zeros)", who);
    const int rc = ds_check(who, n_docs, nq, m, cand_doc, out_score);
    if (rc != 0) return rc < 0 ? rc : SRX_OK;
    if (!rows || !queries || (is_u8 && !u8_scale_min)) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    HIP_TRY(hipSetDevice(device));
    const DenseScoreArgs a = ds_args(rows, u8_scale_min, queries, nullptr, n_docs, dim, nq, doc_base, cand_doc, cand_count, m, out_score);
    if (is_u8)
        launch_rows<true>(a, ds_blocks(a), (hipStream_t)stream_v);
    else
        launch_rows<false>(a, ds_blocks(a), (hipStream_t)stream_v);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

}  // namespace

SRX_API int srx_dense_score_docs_f32(int32_t device, const float *emb, int64_t n_docs, int32_t dim, const float *queries, int32_t nq,
                                     int64_t doc_base, const int32_t *cand_doc, const int32_t *cand_count, int32_t m,
                                     float *out_score, void *stream_v) {
    return dense_score_rows("srx_dense_score_docs_f32", false, device, emb, nullptr, n_docs, dim, queries, nq, doc_base, cand_doc, cand_count, m,
                            out_score, stream_v);
}

SRX_API int srx_dense_score_docs_u8(int32_t device, const uint8_t *corpus, const float *corpus_scales, int64_t n_docs, int32_t dim,
                                    const float *queries, int32_t nq, int64_t doc_base, const int32_t *cand_doc,
                                    const int32_t *cand_count, int32_t m, float *out_score, void *stream_v) {
    return dense_score_rows("srx_dense_score_docs_u8", true, device, corpus, corpus_scales, n_docs, dim, queries, nq, doc_base, cand_doc,
                            cand_count, m, out_score, stream_v);
}

SRX_API int srx_dense_score_docs_i8(int32_t device, const void *corpus, int32_t packed, const float *corpus_scale, int64_t n_docs,
                                    int32_t dim, const int8_t *queries, const float *query_scale, int32_t nq, int64_t doc_base,
                                    const int32_t *cand_doc, const int32_t *cand_count, int32_t m, float *out_score, void *stream_v) {
    const char *who = "srx_dense_score_docs_i8";
    static const int dims[] = {32, 64, 96, 128, 192, 256, 384, 512, 768, 1024};  // the INT8 engine's row lengths
    bool dim_ok = false;
    for (int d : dims) dim_ok = dim_ok || d == dim;
    if (!dim_ok) return fail(SRX_ERR_INVALID, "%s: dim must be 32, 64, 96, 128, 192, 256, 384, 512, 768 or 1024 (pad the rows with zeros)", who);
    if (packed != 0 && packed != 1) return fail(SRX_ERR_INVALID, "%s: packed must be 0 or 1", who);
    const int rc = ds_check(who, n_docs, nq, m, cand_doc, out_score);
    if (rc != 0) return rc < 0 ? rc : SRX_OK;
    if (!corpus || !corpus_scale || !queries || !query_scale) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)corpus | (uintptr_t)queries) & 15) return fail(SRX_ERR_INVALID, "%s: corpus / queries must be 16-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    DenseScoreArgs a = ds_args(corpus, corpus_scale, queries, query_scale, n_docs, dim, nq, doc_base, cand_doc, cand_count, m, out_score);
    a.packed = packed;
    while ((1 << a.glog) < dim / 16) ++a.glog;  // 2 .. 64 lanes per candidate
    // rows in flight per wave: 64 >> glog candidates share a load round, so a chunk of 64 has at most 1 << glog rounds
    const hipStream_t stream = (hipStream_t)stream_v;
    if (a.glog == 1)
        hipLaunchKernelGGL(srx_dense_score_i8_kernel<2>, dim3(ds_blocks(a)), dim3(THREADS), 0, stream, a);
    else if (a.glog == 2)
        hipLaunchKernelGGL(srx_dense_score_i8_kernel<4>, dim3(ds_blocks(a)), dim3(THREADS), 0, stream, a);
    else
        hipLaunchKernelGGL(srx_dense_score_i8_kernel<8>, dim3(ds_blocks(a)), dim3(THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
