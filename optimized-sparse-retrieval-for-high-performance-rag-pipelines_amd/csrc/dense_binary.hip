// dense_binary.hip -- the binary dense index (include/binary/sparse_rx_binary.h): one bit per dimension in 64-row tiles, the
// encoder that writes them, a Hamming top-m search and the distances of given docs.  Replaces nothing in the reference
// project: it has no binary index.
//
// A translation unit of its own (as dense_half.hip is): it is one more user of topk_fold / topk_shrink, and inside another
// file that would change what the compiler inlines into the kernels already there.
//
//   encode    one wave per tile of 64 rows.  For every row of the tile the wave reads 64 consecutive columns (one coalesced
//             256-byte load), compares them with the centre and ballots: the 64 bits are two words of that row, kept by the
//             lane whose number is the row's.  After a step of 128 columns lane r holds four words of row r: one 16-byte
//             store, in the tiled layout (a KiB per wave) or row-major (queries).
//   distance  a wave owns one tile, a lane one doc: its W <= 32 words are loaded once (global_load_dwordx4, a KiB per
//             instruction and wave) and stay in VGPRs while the wave walks a tile of BN_QTILE queries.  A query's words are
//             wave-uniform: scalar loads.  Per 32 dimensions and (doc, query) pair that is one v_xor_b32 with a scalar operand
//             and one accumulating v_bcnt_u32_b32.  The filter's two words for the tile are the lane mask.  Distances go to a
//             u16 matrix [queries of the pass][ld]; 0xFFFF marks a lane that is disallowed or past the end.
//   rank      dense_half.hip's fold loop over a row of that matrix: the ranked value a = dim_pad - dist + 1 >= 1 is exact in
//             fp32 and orders as the distance does, so the helpers that rank (fp32 bits descending, doc ascending) apply as
//             they are; then srx_merge_impl, then a = back to a distance.
//   given     one lane per candidate: its pieces gathered from the tiled layout, the same xor / popcount chain.
#include "filter_common.h"
#include "binary/sparse_rx_binary.h"

namespace {

typedef unsigned bn_v4u __attribute__((ext_vector_type(4)));

constexpr int BN_TILE = 64;      // rows per tile: one per lane
constexpr int BN_QTILE = 128;    // queries a wave walks with its tile's words in registers
constexpr int BN_PASS = 1024;    // queries per pass at most (the distance matrix of a pass lives in the workspace)
constexpr int BN_NPT = 16;       // columns per thread and step of the rank kernel (a chunk of THREADS * BN_NPT = 4096)
constexpr int BN_SPLIT_DOCS = THREADS * BN_NPT * 4;  // a row split is at least this many docs
constexpr unsigned BN_NONE = 0xFFFFu;                // matrix entry of a lane that is not a candidate

inline bool bn_dim_ok(int dim_pad) { return dim_pad >= 128 && dim_pad <= 1024 && dim_pad % 128 == 0; }
inline int64_t bn_tiles(int64_t n_rows) { return (n_rows + BN_TILE - 1) / BN_TILE; }

// ================================================================================================ encode
struct BinEncodeArgs {
    const float *in;      // the chunk's rows (row stride ld elements)
    const float *center;  // f32[dim] or null
    int64_t ld, n_rows;   // rows of this call
    int64_t row0;         // where they sit in the whole set
    int dim, steps;       // steps = dim_pad / 128
    bn_v4u *out;          // the WHOLE set
};

template <bool TILED>
__global__ __launch_bounds__(THREADS) void srx_binary_encode_kernel(BinEncodeArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // tile, relative to row0
    const int64_t t0 = t * BN_TILE;
    if (t0 >= a.n_rows) return;                                   // whole waves leave
    const int live = (int)min((int64_t)BN_TILE, a.n_rows - t0);  // rows of the tile this call holds (>= 1)
    const float *base = a.in + t0 * a.ld;
    for (int s = 0; s < a.steps; ++s) {
        const int c0 = 128 * s + lane, c1 = c0 + 64;
        float m0 = 0.0f, m1 = 0.0f;
        if (a.center != nullptr) {
            if (c0 < a.dim) m0 = a.center[c0];
            if (c1 < a.dim) m1 = a.center[c1];
        }
        unsigned w0 = 0, w1 = 0, w2 = 0, w3 = 0;
        for (int r = 0; r < live; ++r) {  // uniform trip count
            const float *row = base + (int64_t)r * a.ld;
            bool b0 = false, b1 = false;
            if (c0 < a.dim) b0 = row[c0] > m0;  // NaN, -0.0 and equality: false
            if (c1 < a.dim) b1 = row[c1] > m1;
            const unsigned long long lo = __ballot(b0), hi = __ballot(b1);
            if (lane == r) {
                w0 = (unsigned)lo;
                w1 = (unsigned)(lo >> 32);
                w2 = (unsigned)hi;
                w3 = (unsigned)(hi >> 32);
            }
        }
        const bn_v4u piece = {w0, w1, w2, w3};  // rows the call does not hold: zeros
        if constexpr (TILED)
            a.out[(((a.row0 >> 6) + t) * a.steps + s) * 64 + lane] = piece;
        else if (lane < live)
            a.out[(a.row0 + t0 + lane) * a.steps + s] = piece;
    }
}

// ================================================================================================ distances of a pass
struct BinDistArgs {
    const bn_v4u *corpus;
    const uint32_t *q_bits;  // the pass's queries, u32[nq][W]
    int64_t n_docs, ld, n_tiles;
    int nq, n_qtiles;
    const uint32_t *filter_bits;  // null: no filter
    int64_t filter_words;
    const int32_t *q_filter;  // the pass's entries (null: row 0)
    uint16_t *dist;           // [nq][ld]
};

// NJ = W / 4 pieces per doc.  Workgroup b serves query tile b % n_qtiles of tile group b / n_qtiles: the workgroups that read
// one group of docs run together.
template <int NJ>
__global__ __launch_bounds__(THREADS) void srx_binary_dist_kernel(BinDistArgs a) {
    constexpr int W = 4 * NJ;
    const int lane = threadIdx.x & 63;
    const int qt = (int)(blockIdx.x % (unsigned)a.n_qtiles);
    const int64_t tile = (int64_t)(blockIdx.x / (unsigned)a.n_qtiles) * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (tile >= a.n_tiles) return;  // whole waves leave
    const int64_t d = tile * BN_TILE + lane;
    unsigned x[W];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {  // rows past n_docs in the last tile exist in the buffer (zeros)
        const bn_v4u p = a.corpus[(tile * NJ + j) * 64 + lane];
        x[4 * j] = p.x;
        x[4 * j + 1] = p.y;
        x[4 * j + 2] = p.z;
        x[4 * j + 3] = p.w;
    }
    const bool inside = d < a.n_docs;
    const int q_end = min(a.nq, (qt + 1) * BN_QTILE);
    for (int q = qt * BN_QTILE; q < q_end; ++q) {  // uniform
        const SRX_CONSTANT uint32_t *qw = (const SRX_CONSTANT uint32_t *)(a.q_bits + (int64_t)q * W);
        unsigned acc = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) acc += (unsigned)__builtin_popcount(x[w] ^ qw[w]);
        bool allowed = inside;
        if (a.filter_bits != nullptr) {
            const int fr = a.q_filter != nullptr ? cload_i32(a.q_filter + q) : 0;
            if (fr >= 0) {  // uniform; the tile's two words: inside the row (its length is a multiple of 4 words)
                const SRX_CONSTANT uint32_t *frow = (const SRX_CONSTANT uint32_t *)(a.filter_bits + (int64_t)fr * a.filter_words + 2 * tile);
                const unsigned long long mask = (unsigned long long)frow[0] | ((unsigned long long)frow[1] << 32);
                allowed = allowed && ((mask >> lane) & 1ull) != 0ull;
            }
        }
        a.dist[(int64_t)q * a.ld + d] = (uint16_t)(allowed ? acc : BN_NONE);  // d < ld
    }
}

// ================================================================================================ rank
// One workgroup per (query, split of the columns) folds its slice of the distance row into an exact lazy top-m list of
// (a = dim_pad - dist + 1 as fp32 bits, doc).
__global__ __launch_bounds__(THREADS) void srx_binary_topk_kernel(const uint16_t *__restrict__ dist, int64_t ld, int64_t n_docs, int nq, int m,
                                                                  int n_splits, int64_t doc_base, int dim_pad, int32_t *__restrict__ cand_doc,
                                                                  float *__restrict__ cand_score, int32_t *__restrict__ cand_count) {
    __shared__ MergeShared M;
    const int tid = threadIdx.x;
    const int q = blockIdx.x / n_splits, split = blockIdx.x - q * n_splits;
    if (q >= nq) return;
    const int64_t lo = n_docs * split / n_splits, hi = n_docs * (split + 1) / n_splits;
    if (tid == 0) {
        M.tk.count = 0;
        M.tk.tau = 0;
    }
    __syncthreads();
    const uint16_t *row = dist + (int64_t)q * ld;
    for (int64_t c0 = lo; c0 < hi; c0 += (int64_t)THREADS * BN_NPT) {
        unsigned ubits[BN_NPT];
        int udoc[BN_NPT];
        const unsigned tau = M.tk.tau;
#pragma unroll
        for (int n = 0; n < BN_NPT; ++n) {
            const int64_t c = c0 + (int64_t)n * THREADS + tid;
            unsigned dd = BN_NONE;
            if (c < hi) dd = row[c];
            const unsigned b = __float_as_uint((float)(dim_pad + 1 - (int)dd));  // dd <= dim_pad: a >= 1, exact
            ubits[n] = (dd != BN_NONE && b >= tau) ? b : 0u;
            udoc[n] = (int)(doc_base + c);
        }
        topk_fold<BN_NPT, true>(ubits, udoc, m, M.tk, M.hist);
    }
    __syncthreads();
    topk_shrink(m, M.tk, M.hist);
    const unsigned cnt = M.tk.count;
    const int64_t o = (int64_t)blockIdx.x * m;
    for (unsigned i = tid; i < cnt; i += THREADS) {
        cand_doc[o + i] = M.tk.doc[i];
        cand_score[o + i] = __uint_as_float(M.tk.bits[i]);
    }
    if (tid == 0) cand_count[blockIdx.x] = (int)cnt;
}

// the merged rows' values back to distances: entry i of row q is a result iff i < count[q]
__global__ __launch_bounds__(THREADS) void srx_binary_emit_kernel(const float *__restrict__ val, const int32_t *__restrict__ count, int64_t n, int m,
                                                                  int dim_pad, int32_t *__restrict__ out_dist) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t q = i / m;
    out_dist[i] = (int)(i - q * m) < count[q] ? dim_pad + 1 - (int)val[i] : -1;
}

// ================================================================================================ distances of given docs
struct BinDocsArgs {
    const bn_v4u *corpus;
    const uint32_t *q_bits;
    const int32_t *cand_doc, *cand_count;
    int32_t *out_dist;
    int64_t n_docs, doc_base, waves;  // waves = nq * chunks
    int nj, m, chunks;
};
__global__ __launch_bounds__(THREADS) void srx_binary_dist_docs_kernel(BinDocsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= a.waves) return;  // whole waves leave
    const int q = (int)(w / a.chunks);
    const int64_t c = (w - (int64_t)q * a.chunks) * 64 + lane;  // 64 bits: the last chunk of an m near 2^31 ends past int
    int64_t lim = a.m;
    if (a.cand_count != nullptr) lim = min(lim, (int64_t)max(cload_i32(a.cand_count + q), 0));
    int64_t row = -1;  // padding, outside the corpus, beyond m
    if (c < lim) {
        const int64_t local = (int64_t)gload_i32(a.cand_doc + (int64_t)q * a.m + c) - a.doc_base;
        if (local >= 0 && local < a.n_docs) row = local;
    }
    int res = -1;
    if (row >= 0) {
        const bn_v4u *prow = a.corpus + ((row >> 6) * a.nj) * 64 + (row & 63);  // + 64 per piece
        const SRX_CONSTANT bn_v4u *qrow = (const SRX_CONSTANT bn_v4u *)(a.q_bits + (int64_t)q * a.nj * 4);
        unsigned acc = 0;
        for (int j = 0; j < a.nj; ++j) {
            const bn_v4u p = prow[(int64_t)j * 64], u = qrow[j];
            acc += (unsigned)(__builtin_popcount(p.x ^ u.x) + __builtin_popcount(p.y ^ u.y) + __builtin_popcount(p.z ^ u.z) +
                              __builtin_popcount(p.w ^ u.w));
        }
        res = (int)acc;
    }
    if (c < a.m) a.out_dist[(int64_t)q * a.m + c] = res;
}

// ================================================================================================ host side
// the plan of one srx_binary_search call: query passes and row splits as half_common.h's half_plan makes them
struct BinPlan {
    int QB, qb_max;  // queries per pass: as many as keep the u16 matrix within 4 GiB, but 32 .. BN_PASS; of the largest pass
    int64_t ld;      // row length of the distance matrix
    int ns;          // splits of a distance row
};
inline BinPlan bin_plan(int nq, int64_t n_docs, int m) {
    BinPlan p;
    p.ld = bn_tiles(n_docs) * BN_TILE;
    const int64_t q = (4ll << 30) / (p.ld * 2) / 32 * 32;
    p.QB = (int)(q < 32 ? 32 : q > BN_PASS ? BN_PASS : q);
    p.qb_max = nq < p.QB ? nq : p.QB;
    int64_t s = 2048 / (p.qb_max > 0 ? p.qb_max : 1);  // >= 2048 workgroups when the batch is small
    const int64_t by_docs = n_docs / BN_SPLIT_DOCS, cap = (MERGE_NPT * THREADS) / (m > 0 ? m : 1);  // one merge level
    if (s > by_docs) s = by_docs;
    if (s > cap) s = cap;
    p.ns = (int)(s < 1 ? 1 : s);
    return p;
}
struct BinWs {
    uint16_t *dist;  // [qb_max][ld]
    srx_rows cand;   // [qb_max * ns] lists of m
    float *val;      // [qb_max][m]: the merged rows' ranked values
    int64_t bytes;
};
inline BinWs bin_ws(void *base, const BinPlan &pl, int m) {
    BinWs w;
    char *p = (char *)base;
    auto take = [&](int64_t bytes) {
        char *r = p;
        p += (bytes + 255) / 256 * 256;
        return r;
    };
    w.dist = (uint16_t *)take((int64_t)pl.qb_max * pl.ld * 2);
    const int64_t lists = (int64_t)pl.qb_max * pl.ns;
    int32_t *cand_doc = (int32_t *)take(lists * m * 4);
    float *cand_score = (float *)take(lists * m * 4);
    w.cand = srx_plain_rows(cand_doc, cand_score, (int32_t *)take(lists * 4), m);
    w.val = (float *)take((int64_t)pl.qb_max * m * 4);
    w.bytes = (int64_t)(p - (char *)base) + 256;
    return w;
}

void bin_launch_dist(const BinDistArgs &a, int nj, hipStream_t stream) {
    const dim3 grid((unsigned)(((a.n_tiles + WAVES - 1) / WAVES) * a.n_qtiles));  // <= 2^23 * 8
#define SRX_BN(NJ) \
    case NJ: hipLaunchKernelGGL(srx_binary_dist_kernel<NJ>, grid, dim3(THREADS), 0, stream, a); break;
    switch (nj) { SRX_BN(1) SRX_BN(2) SRX_BN(3) SRX_BN(4) SRX_BN(5) SRX_BN(6) SRX_BN(7) SRX_BN(8) }
#undef SRX_BN
}

}  // namespace

SRX_API int64_t srx_binary_bytes(int64_t n_rows, int32_t dim_pad, int32_t tiled) {
    if (n_rows < 0 || !bn_dim_ok(dim_pad) || (tiled != 0 && tiled != 1))
        return fail(SRX_ERR_INVALID, "srx_binary_bytes: need n_rows >= 0, dim_pad a multiple of 128, <= 1024, and tiled 0 or 1%s");
    return (tiled ? bn_tiles(n_rows) * BN_TILE : n_rows) * (int64_t)(dim_pad / 32) * 4;
}

SRX_API int srx_binary_encode(int32_t device, const float *x, int64_t ld, int64_t n_rows, int32_t dim, int32_t dim_pad, int64_t row0,
                              int64_t n_total, const float *center, int32_t tiled, void *out_bits, void *stream_v) {
    const char *who = "srx_binary_encode";
    if (tiled != 0 && tiled != 1) return fail(SRX_ERR_INVALID, "%s: tiled must be 0 or 1", who);
    if (n_rows < 0 || row0 < 0 || n_total < 0) return fail(SRX_ERR_INVALID, "%s: negative count", who);
    if (row0 > n_total || n_rows > n_total - row0) return fail(SRX_ERR_INVALID, "%s: row0 + n_rows > n_total", who);
    if (!bn_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: unsupported dim_pad (a multiple of 128, <= 1024)", who);
    if (dim < 1 || dim > dim_pad || ld < dim) return fail(SRX_ERR_INVALID, "%s: need 1 <= dim <= dim_pad and ld >= dim", who);
    if (tiled && (row0 & 63) != 0) return fail(SRX_ERR_INVALID, "%s: row0 must be a multiple of 64", who);
    if (bn_tiles(n_rows) > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: too many rows in one call", who);
    if (n_rows == 0) return SRX_OK;
    if (!x || !out_bits) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)x | (uintptr_t)center) & 3) return fail(SRX_ERR_INVALID, "%s: input and center must be 4-byte aligned", who);
    if ((uintptr_t)out_bits & 15) return fail(SRX_ERR_INVALID, "%s: out_bits must be 16-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    const BinEncodeArgs a = {x, center, ld, n_rows, row0, dim, dim_pad / 128, (bn_v4u *)out_bits};
    const dim3 grid((unsigned)((bn_tiles(n_rows) + WAVES - 1) / WAVES));
    if (tiled)
        hipLaunchKernelGGL(srx_binary_encode_kernel<true>, grid, dim3(THREADS), 0, (hipStream_t)stream_v, a);
    else
        hipLaunchKernelGGL(srx_binary_encode_kernel<false>, grid, dim3(THREADS), 0, (hipStream_t)stream_v, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int64_t srx_binary_workspace_bytes(int32_t nq, int64_t n_docs, int32_t m) {
    if (nq < 0 || n_docs <= 0 || m <= 0 || m > KMAX) return fail(SRX_ERR_INVALID, "srx_binary_workspace_bytes: bad argument%s");
    return bin_ws(nullptr, bin_plan(nq, n_docs, m), m).bytes;
}

SRX_API int srx_binary_search(int32_t device, const void *bits_tiled, int64_t n_docs, int32_t dim_pad, const uint32_t *q_bits, int32_t nq,
                              int32_t m, int64_t doc_base, const srx_doc_filter *filter, int32_t *out_doc, int32_t *out_dist,
                              int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream_v) {
    const char *who = "srx_binary_search";
    if (filter != nullptr) {
        const int rc = srx_check_filter(who, filter);
        if (rc != SRX_OK) return rc;
    }
    if (nq < 0 || n_docs <= 0 || m <= 0 || m > KMAX) return fail(SRX_ERR_INVALID, "%s: need n_docs > 0, 1 <= m <= 1024", who);
    if (!bn_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 128, <= 1024", who);
    if (doc_base < 0 || doc_base + n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: doc_base + n_docs must fit int32", who);
    if (nq == 0) return SRX_OK;
    if (!bits_tiled || !q_bits || !out_doc || !out_dist || !out_count) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)bits_tiled | (uintptr_t)q_bits) & 15) return fail(SRX_ERR_INVALID, "%s: corpus / queries must be 16-byte aligned", who);
    const BinPlan p = bin_plan(nq, n_docs, m);
    const BinWs w = bin_ws(workspace, p, m);
    if (!workspace || workspace_bytes < w.bytes) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    const int W = dim_pad / 32;
    for (int q0 = 0; q0 < nq; q0 += p.QB) {
        const int qb = nq - q0 < p.QB ? nq - q0 : p.QB;
        const BinDistArgs a = {(const bn_v4u *)bits_tiled, q_bits + (int64_t)q0 * W, n_docs, p.ld, bn_tiles(n_docs), qb, (qb + BN_QTILE - 1) / BN_QTILE,
                               filter ? filter->bits : nullptr, srx_filter_row_words(n_docs),
                               filter && filter->q_filter ? filter->q_filter + q0 : nullptr, w.dist};
        bin_launch_dist(a, W / 4, stream);
        hipLaunchKernelGGL(srx_binary_topk_kernel, dim3((unsigned)((int64_t)qb * p.ns)), dim3(THREADS), 0, stream, (const uint16_t *)w.dist, p.ld, n_docs,
                           qb, (int)m, p.ns, doc_base, (int)dim_pad, w.cand.doc, w.cand.score, w.cand.count);
        HIP_TRY(hipGetLastError());
        const srx_rows out = srx_plain_rows(out_doc + (int64_t)q0 * m, w.val, out_count + q0, m);
        const int rc = srx_merge_impl(device, w.cand, qb, p.ns, m, 0, out, nullptr, 0, stream_v);
        if (rc != SRX_OK) return rc;
        const int64_t n = (int64_t)qb * m;
        hipLaunchKernelGGL(srx_binary_emit_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, (const float *)w.val,
                           (const int32_t *)(out_count + q0), n, (int)m, (int)dim_pad, out_dist + (int64_t)q0 * m);
        HIP_TRY(hipGetLastError());
    }
    return SRX_OK;
}

SRX_API int srx_binary_dist_docs(int32_t device, const void *bits_tiled, int64_t n_docs, int32_t dim_pad, const uint32_t *q_bits, int32_t nq,
                                 int64_t doc_base, const int32_t *cand_doc, const int32_t *cand_count, int32_t m, int32_t *out_dist,
                                 void *stream_v) {
    const char *who = "srx_binary_dist_docs";
    if (!bn_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 128, <= 1024", who);
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if (m < 1) return fail(SRX_ERR_INVALID, "%s: m must be >= 1", who);
    if ((int64_t)nq * (int64_t)m > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: nq * m must fit int32", who);
    if (n_docs <= 0 || n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: n_docs out of range", who);
    if (doc_base < 0) return fail(SRX_ERR_INVALID, "%s: doc_base < 0", who);
    if (nq == 0) return SRX_OK;
    if (!bits_tiled || !q_bits || !cand_doc || !out_dist) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)bits_tiled | (uintptr_t)q_bits) & 15) return fail(SRX_ERR_INVALID, "%s: corpus / queries must be 16-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    const int chunks = (int)(((int64_t)m + 63) / 64);
    const BinDocsArgs a = {(const bn_v4u *)bits_tiled, q_bits, cand_doc, cand_count, out_dist, n_docs, doc_base, (int64_t)nq * chunks, dim_pad / 128, m, chunks};
    const dim3 grid((unsigned)((a.waves + WAVES - 1) / WAVES));  // waves <= nq * m < 2^31
    hipLaunchKernelGGL(srx_binary_dist_docs_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream_v, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
