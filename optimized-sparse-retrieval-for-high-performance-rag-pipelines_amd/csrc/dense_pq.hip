// dense_pq.hip -- the PQ dense index (include/pq/sparse_rx_pq.h): 8-bit product codes in 64-row tiles, the encoder that writes
// them, the per-query score table, the table-lookup scan, the ranking and the scorer of given docs.  Replaces nothing in the
// reference project: it has no PQ index.
//
//   encode    a workgroup = 256 rows (four tiles) x one piece of 16 subspaces, a lane = one row.  Per subspace the codebook
//             (256 x dsub floats, <= 16 KiB) is copied into LDS, the lane keeps its row's dsub columns in registers and walks
//             the 256 codewords four at a time: every lane reads the same LDS address (a broadcast), the four distance
//             chains are independent.  The 16 code bytes are assembled in four registers and leave as one 16-byte store (a
//             KiB per wave) in the tiled layout; the plain layout (training, tests) stores bytes.
//   table     a workgroup = one subspace x up to 16 queries, a thread = one codeword held in registers.  One launch per pass
//             writes the pass's tables to the workspace.
//   scan      the hot path.  A workgroup of 1024 threads serves a group of QG = floor(144 KiB / M KiB) queries: their tables
//             are copied into LDS once, then each of the 16 waves walks its own 64-row tiles (persistent grid, about two
//             workgroups per compute unit in all; LDS admits one per unit at a time; at eight pieces per row the workgroup is
//             512 threads, see pq_scan_threads).  A lane owns one doc of the tile: its
//             M_pad / 16 pieces arrive by coalesced 16-byte loads (a KiB per wave and piece) and stay in VGPRs, the next tile's
//             are in flight while this one is summed.  Per query of the group and m ascending: extract the byte, one
//             ds_read_b32 at m * 256 + code, one v_add_f32.  Codes are read once per query group.  Scores go to the fp32
//             matrix [queries of the pass][ld] in the workspace.
//   rank      the half index's fold (optional filter row, offset applied, > 0) on topk_fold / topk_shrink, then srx_merge_impl.
//   scorer    one workgroup row per query: its table is computed straight into LDS by the function the table kernel uses,
//             lanes walk the candidates, gather the row's pieces from the tiled layout and sum in the same order.
//
// The sum orders are the header's contract: nothing here reorders them to dodge LDS bank conflicts of the byte gathers.
#include "half_common.h"  // the pass plan of a search is the half index's
#include "pq/sparse_rx_pq.h"

namespace {

typedef unsigned pq_v4u __attribute__((ext_vector_type(4)));

constexpr int PQ_TILE = 64;                 // rows per tile: one per lane
constexpr int PQ_MAX_M = 128;               // subspaces at most
constexpr int PQ_SCAN_THREADS = 1024;       // the scan's workgroup: LDS admits one per compute unit, so it is a large one
// ... except at eight pieces per row (M > 112): two tiles of 32 registers do not fit the 128 VGPRs of a 1024-thread workgroup
constexpr int pq_scan_threads(int np) { return np < 8 ? PQ_SCAN_THREADS : PQ_SCAN_THREADS / 2; }
constexpr int PQ_SCAN_FLOATS = 144 * 256;   // the scan's tables in LDS: 144 KiB of the unit's 160
constexpr int PQ_DOCS_FLOATS = PQ_MAX_M * 256;  // the scorer's one table: 128 KiB at M = 128
constexpr int PQ_LUT_Q = 16;                // queries per workgroup of the table kernel
constexpr int PQ_DOCS_CHUNK = 8 * PQ_SCAN_THREADS;  // candidates per workgroup of the scorer before it takes a second one

inline int64_t pq_tiles(int64_t n_rows) { return (n_rows + PQ_TILE - 1) / PQ_TILE; }
inline int pq_pieces(int M) { return (M + 15) / 16; }

// LUT[q][m][c]: the sequential sum from +0.0f over j ascending of fl(q[m dsub + j] * C[m][c][j]); columns at or past dim are zeros
template <int DSUB>
__device__ __forceinline__ float pq_lut_entry(const float *__restrict__ qrow, int m, int dim, const float (&cw)[DSUB]) {
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < DSUB; ++j) {
        const int col = m * DSUB + j;
        const float qv = col < dim ? qrow[col] : 0.0f;
        s = s + qv * cw[j];
    }
    return s;
}
template <int DSUB>
__device__ __forceinline__ void pq_load_codeword(const float *__restrict__ cb, int m, int c, float (&cw)[DSUB]) {
    const hf_v4f *src = reinterpret_cast<const hf_v4f *>(cb + ((int64_t)m * 256 + c) * DSUB);
#pragma unroll
    for (int j = 0; j < DSUB / 4; ++j) {
        const hf_v4f v = src[j];
        cw[4 * j] = v.x; cw[4 * j + 1] = v.y; cw[4 * j + 2] = v.z; cw[4 * j + 3] = v.w;
    }
}
__device__ __forceinline__ unsigned pq_byte(const pq_v4u &piece, int b) { return (piece[b >> 2] >> (8 * (b & 3))) & 255u; }

// ================================================================================================ encode
struct PqEncodeArgs {
    const float *in;      // the chunk's rows (row stride ld elements)
    const float *cb;      // f32[M][256][dsub]
    int64_t ld, n_rows;   // rows of this call
    int64_t row0;         // where they sit in the whole set
    int64_t tiles;        // tiles of this call
    int dim, M, np;       // np = M_pad / 16
    unsigned char *out;   // the WHOLE set
};

template <int DSUB, bool TILED>
__global__ __launch_bounds__(THREADS) void srx_pq_encode_kernel(PqEncodeArgs a) {
    __shared__ __attribute__((aligned(16))) float cb[256 * DSUB];
    const int tid = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * THREADS + tid;  // relative to the chunk
    const bool live = r < a.n_rows;
    const int p = blockIdx.y;
    const float *row = a.in + (live ? r : 0) * a.ld;
    unsigned w[4] = {0u, 0u, 0u, 0u};  // rows the call does not hold and bytes at or past M: zeros
    for (int b = 0; b < 16; ++b) {
        const int m = 16 * p + b;
        if (m >= a.M) break;  // uniform
        __syncthreads();      // the previous subspace's reads are done
        const hf_v4f *src = reinterpret_cast<const hf_v4f *>(a.cb + (int64_t)m * 256 * DSUB);
        for (int i = tid; i < 64 * DSUB; i += THREADS) reinterpret_cast<hf_v4f *>(cb)[i] = src[i];
        __syncthreads();
        float x[DSUB];
#pragma unroll
        for (int j = 0; j < DSUB; ++j) {
            const int col = m * DSUB + j;
            x[j] = (live && col < a.dim) ? row[col] : 0.0f;
        }
        float best = __builtin_inff();
        unsigned code = 0u;
        for (int c = 0; c < 256; c += 4) {
            float d[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < DSUB; ++j)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float t = x[j] - cb[(c + u) * DSUB + j];
                    d[u] = d[u] + t * t;
                }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (d[u] < best) {  // a NaN never wins, a tie keeps the lower code
                    best = d[u];
                    code = (unsigned)(c + u);
                }
        }
        if (!live) code = 0u;
        w[b >> 2] |= code << (8 * (b & 3));
        if constexpr (!TILED)
            if (live) a.out[(a.row0 + r) * a.M + m] = (unsigned char)code;
    }
    if constexpr (TILED) {
        const int64_t t = r >> 6;
        if (t < a.tiles) reinterpret_cast<pq_v4u *>(a.out)[(((a.row0 >> 6) + t) * a.np + p) * 64 + (r & 63)] = (pq_v4u){w[0], w[1], w[2], w[3]};
    }
}

// ================================================================================================ table
struct PqLutArgs {
    const float *cb, *queries;
    int64_t ldq;
    int nq, dim, M;
    float *out;  // [nq][M][256]
};
template <int DSUB>
__global__ __launch_bounds__(THREADS) void srx_pq_lut_kernel(PqLutArgs a) {
    const int m = blockIdx.x, c = threadIdx.x;
    float cw[DSUB];
    pq_load_codeword<DSUB>(a.cb, m, c, cw);
    const int q_end = min(a.nq, ((int)blockIdx.y + 1) * PQ_LUT_Q);
    for (int q = blockIdx.y * PQ_LUT_Q; q < q_end; ++q)
        a.out[((int64_t)q * a.M + m) * 256 + c] = pq_lut_entry<DSUB>(a.queries + (int64_t)q * a.ldq, m, a.dim, cw);
}

// ================================================================================================ scan
struct PqScanArgs {
    const pq_v4u *codes;
    const float *lut;  // the pass's tables [nq][M][256]
    float *scores;     // [nq][ld]
    int64_t n_docs, n_tiles, ld;
    int M, nq, qg, blocks_per_group;  // qg queries per group; workgroup b serves group b / blocks_per_group
};

template <int NP>
__global__ __launch_bounds__(pq_scan_threads(NP)) void srx_pq_scan_kernel(PqScanArgs a) {
    constexpr int NT = pq_scan_threads(NP), NW = NT / 64;
    __shared__ __attribute__((aligned(16))) float lut[PQ_SCAN_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = blockIdx.x / a.blocks_per_group, r = blockIdx.x - g * a.blocks_per_group;
    const int q0 = g * a.qg, nqg = min(a.qg, a.nq - q0), qstride = a.M * 256;
    const hf_v4f *src = reinterpret_cast<const hf_v4f *>(a.lut + (int64_t)q0 * qstride);
    for (int i = tid; i < nqg * a.M * 64; i += NT) reinterpret_cast<hf_v4f *>(lut)[i] = src[i];
    __syncthreads();
    const int64_t stride = (int64_t)a.blocks_per_group * NW;
    int64_t t = (int64_t)r * NW + wave;
    auto load = [&](pq_v4u (&x)[NP], int64_t tile) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < NP; ++p) x[p] = a.codes[(tile * NP + p) * 64 + lane];  // rows past n_docs exist in the buffer (zeros)
    };
    // one step: issue the next tile's loads, then this tile's sums for every query of the group
    auto step = [&](pq_v4u (&cur)[NP], pq_v4u (&nxt)[NP]) __attribute__((always_inline)) {
        const int64_t nt = t + stride;
        if (nt < a.n_tiles) load(nxt, nt);
        const int64_t d = t * PQ_TILE + lane;
        if (d < a.n_docs) {  // the rows past the corpus are never looked up
            for (int qi = 0; qi < nqg; ++qi) {
                const float *L = lut + qi * qstride;
                float acc = 0.0f;
#pragma unroll
                for (int p = 0; p < NP - 1; ++p)
#pragma unroll
                    for (int b = 0; b < 16; ++b) acc = acc + L[(16 * p + b) * 256 + pq_byte(cur[p], b)];
#pragma unroll
                for (int b = 0; b < 16; ++b)
                    if (16 * (NP - 1) + b < a.M) acc = acc + L[(16 * (NP - 1) + b) * 256 + pq_byte(cur[NP - 1], b)];  // uniform
                a.scores[(int64_t)(q0 + qi) * a.ld + d] = acc;
            }
        }
        t = nt;
    };
    pq_v4u b0[NP], b1[NP];
    if (t < a.n_tiles) load(b0, t);
    while (t < a.n_tiles) {
        step(b0, b1);
        if (t >= a.n_tiles) break;
        step(b1, b0);
    }
}

// ================================================================================================ rank
// srx_dense_half_topk_kernel's semantics: one workgroup per (query, split of the columns) folds its slice of the score row into
// an exact lazy top-k list; the ranked value of column c is fl32(score + offset), a result iff > 0 and (with a filter row) bit
// c of the row is set.
__global__ __launch_bounds__(THREADS) void srx_pq_topk_kernel(const float *__restrict__ scores, int64_t ld, int64_t n_docs, int nq, int k,
                                                              int n_splits, int64_t doc_base, float score_offset,
                                                              const uint32_t *__restrict__ filter_bits, int64_t filter_words,
                                                              const int32_t *__restrict__ q_filter, int q0, int32_t *__restrict__ cand_doc,
                                                              float *__restrict__ cand_score, int32_t *__restrict__ cand_count) {
    __shared__ MergeShared M;
    const int tid = threadIdx.x;
    const int q = blockIdx.x / n_splits, split = blockIdx.x - q * n_splits;
    if (q >= nq) return;
    const int64_t lo = n_docs * split / n_splits, hi = n_docs * (split + 1) / n_splits;
    const uint32_t *frow = nullptr;  // null: this query is not filtered
    if (filter_bits != nullptr) {
        const int fr = q_filter != nullptr ? q_filter[q0 + q] : 0;
        if (fr >= 0) frow = filter_bits + (int64_t)fr * filter_words;
    }
    if (tid == 0) {
        M.tk.count = 0;
        M.tk.tau = 0;
    }
    __syncthreads();
    const float *row = scores + (int64_t)q * ld;
    for (int64_t c0 = lo; c0 < hi; c0 += (int64_t)THREADS * HF_NPT) {
        unsigned ubits[HF_NPT];
        int udoc[HF_NPT];
        const unsigned tau = M.tk.tau;
#pragma unroll
        for (int n = 0; n < HF_NPT; ++n) {
            const int64_t c = c0 + (int64_t)n * THREADS + tid;
            float x = 0.0f;
            bool allowed = false;
            if (c < hi) {  // c < n_docs: the filter row has a word for it
                x = row[c] + score_offset;  // + 0.0f by default (exact)
                allowed = frow == nullptr || ((frow[c >> 5] >> (c & 31)) & 1u) != 0u;
            }
            const unsigned b = __float_as_uint(x);
            ubits[n] = (allowed && x > 0.0f && b >= tau) ? b : 0u;
            udoc[n] = (int)(doc_base + c);
        }
        topk_fold<HF_NPT, true>(ubits, udoc, k, M.tk, M.hist);
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

// ================================================================================================ scorer of given docs
struct PqDocsArgs {
    const pq_v4u *codes;
    const float *cb, *queries;
    const int32_t *cand_doc, *cand_count;
    float *out_score;
    int64_t n_docs, doc_base, ldq;
    int dim, M, np, m;
};
template <int DSUB>
__global__ __launch_bounds__(PQ_SCAN_THREADS) void srx_pq_score_docs_kernel(PqDocsArgs a) {
    __shared__ float lut[PQ_DOCS_FLOATS];
    const int tid = threadIdx.x, q = blockIdx.x;
    const float *qrow = a.queries + (int64_t)q * a.ldq;
    for (int i = tid; i < a.M * 256; i += PQ_SCAN_THREADS) {
        float cw[DSUB];
        pq_load_codeword<DSUB>(a.cb, i >> 8, i & 255, cw);
        lut[i] = pq_lut_entry<DSUB>(qrow, i >> 8, a.dim, cw);
    }
    __syncthreads();
    int64_t lim = a.m;
    if (a.cand_count != nullptr) lim = min(lim, (int64_t)max(gload_i32(a.cand_count + q), 0));
    for (int64_t c = (int64_t)blockIdx.y * PQ_SCAN_THREADS + tid; c < a.m; c += (int64_t)gridDim.y * PQ_SCAN_THREADS) {
        int64_t row = -1;  // padding, outside the corpus
        if (c < lim) {
            const int64_t local = (int64_t)gload_i32(a.cand_doc + (int64_t)q * a.m + c) - a.doc_base;
            if (local >= 0 && local < a.n_docs) row = local;
        }
        float res = 0.0f;
        if (row >= 0) {
            const pq_v4u *prow = a.codes + ((row >> 6) * a.np) * 64 + (row & 63);  // + 64 per piece
            float acc = 0.0f;
            for (int p = 0; p < a.np; ++p) {
                const pq_v4u piece = prow[(int64_t)p * 64];
#pragma unroll
                for (int b = 0; b < 16; ++b)
                    if (16 * p + b < a.M) acc = acc + lut[(16 * p + b) * 256 + pq_byte(piece, b)];  // the search's chain
            }
            res = acc;
        }
        a.out_score[(int64_t)q * a.m + c] = res;
    }
}

// ================================================================================================ host side
// the geometry of a call: dsub in {4, 8, 16}, 1 <= dim <= 1024, M = ceil(dim / dsub) <= 128
int pq_geometry(const char *who, int32_t dim, int32_t dsub, int *M) {
    if (dsub != 4 && dsub != 8 && dsub != 16) return fail(SRX_ERR_INVALID, "%s: dsub must be 4, 8 or 16", who);
    if (dim < 1 || dim > 1024) return fail(SRX_ERR_INVALID, "%s: need 1 <= dim <= 1024", who);
    *M = (dim + dsub - 1) / dsub;
    if (*M > PQ_MAX_M) return fail(SRX_ERR_INVALID, "%s: M = ceil(dim / dsub) must be <= 128", who);
    return SRX_OK;
}

struct PqWs {
    float *lut;     // [qb_max][M][256]
    float *scores;  // [qb_max][ld]
    srx_rows cand;  // [qb_max * ns] lists of k
    int64_t bytes;
};
inline PqWs pq_ws(void *base, const HalfPlan &pl, int M, int k) {
    PqWs w;
    char *p = (char *)base;
    auto take = [&](int64_t bytes) {
        char *r = p;
        p += (bytes + 255) / 256 * 256;
        return r;
    };
    w.lut = (float *)take((int64_t)pl.qb_max * M * 1024);
    w.scores = (float *)take((int64_t)pl.qb_max * pl.ld * 4);
    const int64_t lists = (int64_t)pl.qb_max * pl.ns;
    int32_t *cand_doc = (int32_t *)take(lists * k * 4);
    float *cand_score = (float *)take(lists * k * 4);
    w.cand = srx_plain_rows(cand_doc, cand_score, (int32_t *)take(lists * 4), k);
    w.bytes = (int64_t)(p - (char *)base) + 256;
    return w;
}

template <bool TILED>
void pq_launch_encode(const PqEncodeArgs &a, int dsub, hipStream_t stream) {
    const dim3 grid((unsigned)((a.tiles * PQ_TILE + THREADS - 1) / THREADS), (unsigned)a.np);
    switch (dsub) {
    case 4: hipLaunchKernelGGL((srx_pq_encode_kernel<4, TILED>), grid, dim3(THREADS), 0, stream, a); break;
    case 8: hipLaunchKernelGGL((srx_pq_encode_kernel<8, TILED>), grid, dim3(THREADS), 0, stream, a); break;
    default: hipLaunchKernelGGL((srx_pq_encode_kernel<16, TILED>), grid, dim3(THREADS), 0, stream, a); break;
    }
}
void pq_launch_lut(const PqLutArgs &a, int dsub, hipStream_t stream) {
    const dim3 grid((unsigned)a.M, (unsigned)((a.nq + PQ_LUT_Q - 1) / PQ_LUT_Q));
    switch (dsub) {
    case 4: hipLaunchKernelGGL(srx_pq_lut_kernel<4>, grid, dim3(THREADS), 0, stream, a); break;
    case 8: hipLaunchKernelGGL(srx_pq_lut_kernel<8>, grid, dim3(THREADS), 0, stream, a); break;
    default: hipLaunchKernelGGL(srx_pq_lut_kernel<16>, grid, dim3(THREADS), 0, stream, a); break;
    }
}
void pq_launch_scan(const PqScanArgs &a, int n_groups, hipStream_t stream) {
    const dim3 grid((unsigned)(n_groups * a.blocks_per_group));
#define SRX_PQ(NP) \
    case NP: hipLaunchKernelGGL(srx_pq_scan_kernel<NP>, grid, dim3(pq_scan_threads(NP)), 0, stream, a); break;
    switch (pq_pieces(a.M)) { SRX_PQ(1) SRX_PQ(2) SRX_PQ(3) SRX_PQ(4) SRX_PQ(5) SRX_PQ(6) SRX_PQ(7) SRX_PQ(8) }
#undef SRX_PQ
}

}  // namespace

SRX_API int64_t srx_pq_bytes(int64_t n_rows, int32_t M) {
    if (n_rows < 0 || M < 1 || M > PQ_MAX_M) return fail(SRX_ERR_INVALID, "srx_pq_bytes: need n_rows >= 0 and 1 <= M <= 128%s");
    return pq_tiles(n_rows) * PQ_TILE * (int64_t)(pq_pieces(M) * 16);
}

SRX_API int srx_pq_encode(int32_t device, const float *x, int64_t ld, int64_t n_rows, int32_t dim, int32_t dsub, int64_t row0, int64_t n_total,
                          const float *codebooks, int32_t tiled, void *out_codes, void *stream_v) {
    const char *who = "srx_pq_encode";
    int M = 0;
    const int rc = pq_geometry(who, dim, dsub, &M);
    if (rc != SRX_OK) return rc;
    if (tiled != 0 && tiled != 1) return fail(SRX_ERR_INVALID, "%s: tiled must be 0 or 1", who);
    if (n_rows < 0 || row0 < 0 || n_total < 0) return fail(SRX_ERR_INVALID, "%s: negative count", who);
    if (row0 > n_total || n_rows > n_total - row0) return fail(SRX_ERR_INVALID, "%s: row0 + n_rows > n_total", who);
    if (ld < dim) return fail(SRX_ERR_INVALID, "%s: need ld >= dim", who);
    if (tiled && (row0 & 63) != 0) return fail(SRX_ERR_INVALID, "%s: row0 must be a multiple of 64", who);
    if (pq_tiles(n_rows) > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: too many rows in one call", who);
    if (n_rows == 0) return SRX_OK;
    if (!x || !codebooks || !out_codes) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)x & 3) return fail(SRX_ERR_INVALID, "%s: input must be 4-byte aligned", who);
    if ((uintptr_t)codebooks & 15) return fail(SRX_ERR_INVALID, "%s: codebooks must be 16-byte aligned", who);
    if (tiled && ((uintptr_t)out_codes & 15)) return fail(SRX_ERR_INVALID, "%s: out_codes must be 16-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    const PqEncodeArgs a = {x, codebooks, ld, n_rows, row0, pq_tiles(n_rows), dim, M, pq_pieces(M), (unsigned char *)out_codes};
    if (tiled)
        pq_launch_encode<true>(a, dsub, (hipStream_t)stream_v);
    else
        pq_launch_encode<false>(a, dsub, (hipStream_t)stream_v);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int srx_pq_lut(int32_t device, const float *codebooks, int32_t dim, int32_t dsub, const float *queries, int64_t ldq, int32_t nq,
                       float *out_lut, void *stream_v) {
    const char *who = "srx_pq_lut";
    int M = 0;
    const int rc = pq_geometry(who, dim, dsub, &M);
    if (rc != SRX_OK) return rc;
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if (ldq < dim) return fail(SRX_ERR_INVALID, "%s: need ldq >= dim", who);
    if (nq == 0) return SRX_OK;
    if (!codebooks || !queries || !out_lut) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)queries & 3) return fail(SRX_ERR_INVALID, "%s: queries must be 4-byte aligned", who);
    if (((uintptr_t)codebooks | (uintptr_t)out_lut) & 15) return fail(SRX_ERR_INVALID, "%s: codebooks / out_lut must be 16-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    pq_launch_lut({codebooks, queries, ldq, nq, dim, M, out_lut}, dsub, (hipStream_t)stream_v);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int64_t srx_pq_workspace_bytes(int32_t nq, int64_t n_docs, int32_t M, int32_t k) {
    if (nq < 0 || n_docs <= 0 || M < 1 || M > PQ_MAX_M || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "srx_pq_workspace_bytes: bad argument%s");
    return pq_ws(nullptr, half_plan(nq, n_docs, k), M, k).bytes;
}

SRX_API int srx_pq_search(int32_t device, const void *codes, int64_t n_docs, int32_t dim, int32_t dsub, const float *codebooks, const float *queries,
                          int64_t ldq, int32_t nq, int32_t k, int64_t doc_base, const srx_doc_filter *filter, int32_t *out_doc, float *out_score,
                          int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream_v, float score_offset) {
    const char *who = "srx_pq_search";
    int M = 0;
    int rc = pq_geometry(who, dim, dsub, &M);
    if (rc != SRX_OK) return rc;
    if (filter != nullptr) {
        rc = srx_check_filter(who, filter);
        if (rc != SRX_OK) return rc;
    }
    if (nq < 0 || n_docs <= 0 || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "%s: need n_docs > 0, 1 <= k <= 1024", who);
    if (ldq < dim) return fail(SRX_ERR_INVALID, "%s: need ldq >= dim", who);
    if (doc_base < 0 || doc_base + n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: doc_base + n_docs must fit int32", who);
    if (nq == 0) return SRX_OK;
    if (!codes || !codebooks || !queries || !out_doc || !out_score || !out_count) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)codes | (uintptr_t)codebooks) & 15) return fail(SRX_ERR_INVALID, "%s: codes / codebooks must be 16-byte aligned", who);
    if ((uintptr_t)queries & 3) return fail(SRX_ERR_INVALID, "%s: queries must be 4-byte aligned", who);
    const HalfPlan p = half_plan(nq, n_docs, k);
    const PqWs w = pq_ws(workspace, p, M, k);
    if (!workspace || workspace_bytes < w.bytes) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    HIP_TRY(hipSetDevice(device));
    int n_cus = 0;
    HIP_TRY(hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, device));
    hipStream_t stream = (hipStream_t)stream_v;
    const uint32_t *fbits = filter ? filter->bits : nullptr;
    const int32_t *qf = filter ? filter->q_filter : nullptr;
    const int64_t n_tiles = pq_tiles(n_docs);
    const int qg_max = PQ_SCAN_FLOATS / (M * 256);  // >= 1: M <= 128
    for (int q0 = 0; q0 < nq; q0 += p.QB) {
        const int qb = nq - q0 < p.QB ? nq - q0 : p.QB;
        pq_launch_lut({codebooks, queries + (int64_t)q0 * ldq, ldq, qb, dim, M, w.lut}, dsub, stream);
        const int qg = qb < qg_max ? qb : qg_max, n_groups = (qb + qg - 1) / qg;
        // a persistent grid of about two workgroups per compute unit, at most one per tile of each wave, at least one per group
        int64_t bpg = (2 * (int64_t)(n_cus > 0 ? n_cus : 1) + n_groups - 1) / n_groups;
        const int n_waves = pq_scan_threads(pq_pieces(M)) / 64;
        const int64_t by_tiles = (n_tiles + n_waves - 1) / n_waves;
        if (bpg > by_tiles) bpg = by_tiles;
        const PqScanArgs a = {(const pq_v4u *)codes, w.lut, w.scores, n_docs, n_tiles, p.ld, M, qb, qg, (int)(bpg < 1 ? 1 : bpg)};
        pq_launch_scan(a, n_groups, stream);
        hipLaunchKernelGGL(srx_pq_topk_kernel, dim3((unsigned)((int64_t)qb * p.ns)), dim3(THREADS), 0, stream, (const float *)w.scores, p.ld, n_docs, qb,
                           (int)k, p.ns, doc_base, score_offset, fbits, srx_filter_row_words(n_docs), qf, q0, w.cand.doc, w.cand.score, w.cand.count);
        HIP_TRY(hipGetLastError());
        const srx_rows out = srx_plain_rows(out_doc + (int64_t)q0 * k, out_score + (int64_t)q0 * k, out_count + q0, k);
        rc = srx_merge_impl(device, w.cand, qb, p.ns, k, 0, out, nullptr, 0, stream_v);
        if (rc != SRX_OK) return rc;
    }
    return SRX_OK;
}

SRX_API int srx_pq_score_docs(int32_t device, const void *codes, int64_t n_docs, int32_t dim, int32_t dsub, const float *codebooks, const float *queries,
                              int64_t ldq, int32_t nq, int64_t doc_base, const int32_t *cand_doc, const int32_t *cand_count, int32_t m,
                              float *out_score, void *stream_v) {
    const char *who = "srx_pq_score_docs";
    int M = 0;
    const int rc = pq_geometry(who, dim, dsub, &M);
    if (rc != SRX_OK) return rc;
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if (m < 1) return fail(SRX_ERR_INVALID, "%s: m must be >= 1", who);
    if ((int64_t)nq * (int64_t)m > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: nq * m must fit int32", who);
    if (n_docs <= 0 || n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: n_docs out of range", who);
    if (ldq < dim) return fail(SRX_ERR_INVALID, "%s: need ldq >= dim", who);
    if (doc_base < 0) return fail(SRX_ERR_INVALID, "%s: doc_base < 0", who);
    if (nq == 0) return SRX_OK;
    if (!codes || !codebooks || !queries || !cand_doc || !out_score) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)codes | (uintptr_t)codebooks) & 15) return fail(SRX_ERR_INVALID, "%s: codes / codebooks must be 16-byte aligned", who);
    if ((uintptr_t)queries & 3) return fail(SRX_ERR_INVALID, "%s: queries must be 4-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    const PqDocsArgs a = {(const pq_v4u *)codes, codebooks, queries, cand_doc, cand_count, out_score, n_docs, doc_base, ldq, dim, M, pq_pieces(M), m};
    const int64_t chunks = ((int64_t)m + PQ_DOCS_CHUNK - 1) / PQ_DOCS_CHUNK;
    const dim3 grid((unsigned)nq, (unsigned)(chunks < 64 ? chunks : 64));
    switch (dsub) {
    case 4: hipLaunchKernelGGL(srx_pq_score_docs_kernel<4>, grid, dim3(PQ_SCAN_THREADS), 0, (hipStream_t)stream_v, a); break;
    case 8: hipLaunchKernelGGL(srx_pq_score_docs_kernel<8>, grid, dim3(PQ_SCAN_THREADS), 0, (hipStream_t)stream_v, a); break;
    default: hipLaunchKernelGGL(srx_pq_score_docs_kernel<16>, grid, dim3(PQ_SCAN_THREADS), 0, (hipStream_t)stream_v, a); break;
    }
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
