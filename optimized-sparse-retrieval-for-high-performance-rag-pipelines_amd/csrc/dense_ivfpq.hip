// dense_ivfpq.hip -- the IVF-PQ dense index (include/ivfpq/sparse_rx_ivfpq.h): product codes of the residual x - centroid in
// k-means lists.  Replaces nothing in the reference project: it has no clustered and no quantised index.
//
//   encode    the PQ encoder's shape with a gather and a subtraction in front: a workgroup = 256 packed rows x one piece of 16
//             subspaces, a lane = one row; per subspace the codebook sits in LDS, the lane's dsub residual columns
//             fl(x - rounded centroid) sit in registers, four distance chains walk the 256 codewords.
//   probe     srx_ivf_probe_pass of dense_ivf.hip (ivf_probe.h): it leaves EVERY centroid's score, the coarse terms.
//   table     srx_pq_lut, the PQ index's own table kernel, on the residual codebooks: LUT[P][M][256] in the workspace.
//   prepare   one workgroup per query: the probe row cleaned; per slot the list's first tile, its coarse term and the running
//             tile count (the prefix sum the slices are cut from).
//   scan      the hot path; a work item is (query, slice of the query's concatenated tiles).  The workgroup copies the query's
//             table into LDS once (static, 16 KiB per piece of a row: LDS admits 10 .. 1 workgroups per compute unit, see
//             ivfpq_scan_threads), its waves take alternate tiles of the slice.  A lane owns one row: its pieces arrive by
//             coalesced 16-byte loads and stay in VGPRs, the next tile's are in flight while this one is summed -- the next
//             tile is found through the prefix sums with scalar loads, so a list boundary costs no vector work.  Per subspace:
//             one byte extract, one ds_read_b32, one v_add_f32.  The epilogue adds the tile's (scalar) coarse term and stores the
//             wave's 64 scores into the (query, slice) strip.
//   rank      the IVF index's fold over a strip (filter on row_doc, offset, > 0), then srx_merge_impl over a query's S lists.
//             There is no top-k fused into the scan.
//   scorer    doc -> doc_row -> tile_list; the coarse term by srx_dense_score_docs_half over the centroid corpus; then one
//             workgroup row per query computes its table into LDS and adds the code sums in the search's order.
#include "half_common.h"
#include "ivf_probe.h"
#include "ivfpq/sparse_rx_ivfpq.h"
#include "pq/sparse_rx_pq.h"

namespace {

typedef unsigned pq_v4u __attribute__((ext_vector_type(4)));

constexpr int IVFPQ_TILE = 64, IVFPQ_MAX_M = 128, IVFPQ_MAX_LIST = 65536, IVFPQ_MAX_PROBE = 1024, IVFPQ_PASS = 1024;
constexpr int64_t IVFPQ_MAX_TILES = 1ll << 25;
constexpr int64_t IVFPQ_MAX_QUERY_TILES = 1ll << 26;  // nprobe * max_list_tiles: a query's running tile counts are 32-bit
constexpr int IVFPQ_NPT = 4;            // columns per thread and step of the rank kernel
constexpr int IVFPQ_DOCS_THREADS = 1024;  // the scorer's workgroup: its table is up to 128 KiB, one workgroup per compute unit
constexpr int IVFPQ_DOCS_CHUNK = 8 * IVFPQ_DOCS_THREADS;
// The scan's workgroup by pieces per row.  The table is static LDS of 16 KiB per piece, so 160 KiB admit 10, 5, 3, 2, 2, 1, 1, 1
// workgroups per compute unit.  Up to two pieces several small workgroups share a unit (256 threads: a short slice wastes few
// waves); at six and seven pieces the unit's one workgroup brings all 16 waves a 128-VGPR budget allows; at eight pieces two
// tiles of 32 registers do not fit that budget, and from three to five the unit already holds two or three workgroups.
constexpr int ivfpq_scan_threads(int np) { return np <= 2 ? 256 : (np == 6 || np == 7) ? 1024 : 512; }

inline int ivfpq_pieces(int M) { return (M + 15) / 16; }
inline int64_t r256(int64_t x) { return (x + 255) / 256 * 256; }
bool type_ok(int32_t type) { return type == SRX_HALF_F16 || type == SRX_HALF_BF16; }

__device__ __forceinline__ unsigned pq_byte(const pq_v4u &piece, int b) { return (piece[b >> 2] >> (8 * (b & 3))) & 255u; }

// the f32 value of column `col` of packed centroid row c (fragment order: 8 halves per piece)
template <int TYPE>
__device__ __forceinline__ float ivfpq_centroid(const unsigned short *__restrict__ cent, int c, int ks, int col) {
    const unsigned short u = cent[hf_piece(c, ks, col >> 4, (col >> 3) & 1) * 8 + (col & 7)];
    if constexpr (TYPE == SRX_HALF_F16)
        return (float)__builtin_bit_cast(_Float16, u);
    else
        return __uint_as_float((unsigned)u << 16);
}

// ================================================================================================ encode
struct IvfpqEncodeArgs {
    const float *in;             // f32[n_src][ld]
    const float *cb;             // f32[M][256][dsub]
    const unsigned short *cent;  // packed half centroids
    const int32_t *src_row, *row_list;
    int64_t ld, n_src, n_rows;   // packed rows of this call
    int64_t tile0, tiles;        // the first tile it covers, how many
    int dim, M, np, ks, nlist;
    pq_v4u *out;                 // the WHOLE permuted buffer
};

template <int DSUB, int TYPE>
__global__ __launch_bounds__(THREADS) void srx_ivfpq_encode_kernel(IvfpqEncodeArgs a) {
    __shared__ __attribute__((aligned(16))) float cb[256 * DSUB];
    const int tid = threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * THREADS + tid;  // relative to the chunk
    const int p = blockIdx.y;
    int64_t src = -1;
    int list = 0;
    if (r < a.n_rows) {
        src = gload_i32(a.src_row + r);
        list = gload_i32(a.row_list + r);
    }
    const bool live = src >= 0 && src < a.n_src && list >= 0 && list < a.nlist;  // anything else is padding: zero codes
    const float *row = a.in + (live ? src : 0) * a.ld;
    unsigned w[4] = {0u, 0u, 0u, 0u};
    for (int b = 0; b < 16; ++b) {
        const int m = 16 * p + b;
        if (m >= a.M) break;  // uniform
        __syncthreads();      // the previous subspace's reads are done
        const hf_v4f *cbsrc = reinterpret_cast<const hf_v4f *>(a.cb + (int64_t)m * 256 * DSUB);
        for (int i = tid; i < 64 * DSUB; i += THREADS) reinterpret_cast<hf_v4f *>(cb)[i] = cbsrc[i];
        __syncthreads();
        float x[DSUB];
#pragma unroll
        for (int j = 0; j < DSUB; ++j) {
            const int col = m * DSUB + j;
            x[j] = (live && col < a.dim) ? row[col] - ivfpq_centroid<TYPE>(a.cent, list, a.ks, col) : 0.0f;  // the residual
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
    }
    const int64_t t = r >> 6;
    if (t < a.tiles) a.out[((a.tile0 + t) * a.np + p) * 64 + (r & 63)] = (pq_v4u){w[0], w[1], w[2], w[3]};
}

// ================================================================================================ prepare
// The slots of a query: slot j is the j-th entry of its probe row.  A slot that is padding, out of range or a repeat has no tile.
struct IvfpqPrepArgs {
    const int32_t *probe_list;  // [P][nprobe]
    const int32_t *list_tile;
    const float *cscores;       // [P][ldc]
    int32_t *tstart;            // [P][nprobe]: the slot's first tile
    float *coarse;              // [P][nprobe]: its coarse term
    int32_t *pre;               // [P][nprobe + 1]: tiles of the slots before it; pre[nprobe] = the query's tiles
    int64_t ldc, n_tiles, max_list_tiles;
    int nprobe, nlist;
};
__global__ __launch_bounds__(THREADS) void srx_ivfpq_prepare_kernel(IvfpqPrepArgs a) {
    __shared__ int L[IVFPQ_MAX_PROBE], len[IVFPQ_MAX_PROBE], part[THREADS];
    const int tid = threadIdx.x, q = blockIdx.x;
    const int64_t base = (int64_t)q * a.nprobe;
    for (int j = tid; j < a.nprobe; j += THREADS) L[j] = a.probe_list[base + j];
    __syncthreads();
    for (int j = tid; j < a.nprobe; j += THREADS) {
        const int c = L[j];
        bool ok = c >= 0 && c < a.nlist;
        for (int i = 0; ok && i < j; ++i) ok = L[i] != c;
        int64_t t_lo = 0, n = 0;
        float co = 0.0f;
        if (ok) {
            t_lo = max(a.list_tile[c], 0);
            const int64_t t_hi = min(min((int64_t)a.list_tile[c + 1], a.n_tiles), t_lo + a.max_list_tiles);
            n = t_hi > t_lo ? t_hi - t_lo : 0;
            co = a.cscores[(int64_t)q * a.ldc + c];
        }
        len[j] = (int)n;
        a.tstart[base + j] = (int)t_lo;
        a.coarse[base + j] = co;
    }
    __syncthreads();
    // exclusive prefix: thread t owns slots 4 t .. 4 t + 3 (nprobe <= 1024)
    int s = 0;
    for (int u = 0; u < 4; ++u)
        if (4 * tid + u < a.nprobe) s += len[4 * tid + u];
    part[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int i = 0; i < THREADS; ++i) {
            const int v = part[i];
            part[i] = acc;
            acc += v;
        }
    }
    __syncthreads();
    int32_t *pre = a.pre + (int64_t)q * (a.nprobe + 1);
    s = part[tid];
    for (int u = 0; u < 4; ++u)
        if (4 * tid + u < a.nprobe) {
            pre[4 * tid + u] = s;
            s += len[4 * tid + u];
        }
    if (4 * tid < a.nprobe && 4 * tid + 4 >= a.nprobe) pre[a.nprobe] = s;  // the thread that owns the last slot
}

// the slice `s` of a query with `total` tiles: tiles [g0, g1) of its concatenation
__device__ __forceinline__ void ivfpq_slice(int total, int S, int s, int &g0, int &g1) {
    const int per = (total + S - 1) / S;
    g0 = min(s * per, total);
    g1 = min(g0 + per, total);
}

// ================================================================================================ scan
struct IvfpqScanArgs {
    const pq_v4u *codes;
    const float *lut;        // [P][M][256]
    const int32_t *pre, *tstart;
    const float *coarse;
    float *strips;           // [P * S][L * 64]
    int32_t *strip_tile;     // [P * S][L]: the packed tile of a strip tile
    int64_t L;               // tiles a slice holds at most
    int M, nprobe, S;
};

template <int NP>
__global__ __launch_bounds__(ivfpq_scan_threads(NP)) void srx_ivfpq_scan_kernel(IvfpqScanArgs a) {
    constexpr int NT = ivfpq_scan_threads(NP), NW = NT / 64;
    __shared__ __attribute__((aligned(16))) float lut[NP * 16 * 256];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int q = blockIdx.x / a.S, s = blockIdx.x - q * a.S;
    const int32_t *pre = a.pre + (int64_t)q * (a.nprobe + 1);
    const int32_t *tstart = a.tstart + (int64_t)q * a.nprobe;
    const float *coarse = a.coarse + (int64_t)q * a.nprobe;
    int g0, g1;
    ivfpq_slice(pre[a.nprobe], a.S, s, g0, g1);
    if (g0 >= g1) return;  // uniform: an empty slice copies no table
    int g = g0 + wave;     // this wave's tile of the concatenation; uniform
    int j = 0;             // the slot with pre[j] <= g < pre[j + 1]: found once, then only advanced
    {
        int hi = a.nprobe;
        const int gg = min(g, g1 - 1);
        while (hi - j > 1) {  // pre[j] <= gg < pre[hi]
            const int mid = (j + hi) >> 1;
            if (pre[mid] <= gg) j = mid; else hi = mid;
        }
    }
    // tile gi (< g1) of the concatenation: its packed tile and coarse term; advances j past the slots that end before it
    auto locate = [&](int gi, int64_t &tile, float &co) __attribute__((always_inline)) {
        while (pre[j + 1] <= gi) ++j;  // gi < pre[nprobe]: ends at j < nprobe
        tile = (int64_t)tstart[j] + (gi - pre[j]);
        co = coarse[j];
    };
    auto load = [&](pq_v4u (&x)[NP], int64_t tile) __attribute__((always_inline)) {
#pragma unroll
        for (int p = 0; p < NP; ++p) x[p] = a.codes[(tile * NP + p) * 64 + lane];  // padding rows exist in the buffer (zero codes)
    };
    int64_t tile = 0;
    float co = 0.0f;
    pq_v4u b0[NP], b1[NP];
    if (g < g1) {
        locate(g, tile, co);
        load(b0, tile);  // in flight over the table copy
    }
    const hf_v4f *src = reinterpret_cast<const hf_v4f *>(a.lut + (int64_t)q * a.M * 256);
    for (int i = tid; i < a.M * 64; i += NT) reinterpret_cast<hf_v4f *>(lut)[i] = src[i];
    __syncthreads();
    float *strip = a.strips + (int64_t)blockIdx.x * a.L * 64;
    int32_t *stile = a.strip_tile + (int64_t)blockIdx.x * a.L;
    // one step: issue the next tile's loads, then this tile's sums
    auto step = [&](pq_v4u (&cur)[NP], pq_v4u (&nxt)[NP]) __attribute__((always_inline)) {
        const int ng = g + NW;
        int64_t ntile = 0;
        float nco = 0.0f;
        if (ng < g1) {
            locate(ng, ntile, nco);
            load(nxt, ntile);
        }
        float acc = 0.0f;
#pragma unroll
        for (int p = 0; p < NP - 1; ++p)
#pragma unroll
            for (int b = 0; b < 16; ++b) acc = acc + lut[(16 * p + b) * 256 + pq_byte(cur[p], b)];
#pragma unroll
        for (int b = 0; b < 16; ++b)
            if (16 * (NP - 1) + b < a.M) acc = acc + lut[(16 * (NP - 1) + b) * 256 + pq_byte(cur[NP - 1], b)];  // uniform
        strip[(int64_t)(g - g0) * 64 + lane] = co + acc;  // g - g0 < L
        if (lane == 0) stile[g - g0] = (int)tile;
        g = ng;
        tile = ntile;
        co = nco;
    };
    while (g < g1) {
        step(b0, b1);
        if (g >= g1) break;
        step(b1, b0);
    }
}

// ================================================================================================ rank
// one workgroup per (query, slice): the strip folded into an exact list of k (unordered) for the merge
struct IvfpqRankArgs {
    const float *strips;
    const int32_t *strip_tile, *pre, *row_doc;
    const uint32_t *filter_bits;
    const int32_t *q_filter;
    int32_t *cand_doc;
    float *cand_score;
    int32_t *cand_count;
    int64_t L, n_docs, doc_base, filter_words;
    int nprobe, S, k, q0;
    float score_offset;
};
__global__ __launch_bounds__(THREADS) void srx_ivfpq_rank_kernel(IvfpqRankArgs a) {
    __shared__ MergeShared M;
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int q = (int)(p / a.S), s = (int)(p - (int64_t)q * a.S);
    int g0, g1;
    ivfpq_slice(a.pre[(int64_t)q * (a.nprobe + 1) + a.nprobe], a.S, s, g0, g1);
    const int64_t cols = (int64_t)(g1 - g0) * 64;
    const uint32_t *frow = nullptr;
    if (a.filter_bits != nullptr) {
        const int fr = a.q_filter != nullptr ? a.q_filter[a.q0 + q] : 0;
        if (fr >= 0) frow = a.filter_bits + (int64_t)fr * a.filter_words;
    }
    if (tid == 0) {
        M.tk.count = 0;
        M.tk.tau = 0;
    }
    __syncthreads();
    const float *row = a.strips + p * a.L * 64;
    const int32_t *stile = a.strip_tile + p * a.L;
    for (int64_t c0 = 0; c0 < cols; c0 += THREADS * IVFPQ_NPT) {
        unsigned ubits[IVFPQ_NPT];
        int udoc[IVFPQ_NPT];
        const unsigned tau = M.tk.tau;
#pragma unroll
        for (int n = 0; n < IVFPQ_NPT; ++n) {
            const int64_t col = c0 + n * THREADS + tid;
            float x = 0.0f;
            int doc = -1;
            if (col < cols) {
                doc = a.row_doc[(int64_t)stile[col >> 6] * 64 + (col & 63)];
                x = row[col] + a.score_offset;
            }
            bool allowed = doc >= 0 && doc < a.n_docs;
            if (allowed && frow != nullptr) allowed = ((frow[doc >> 5] >> (doc & 31)) & 1u) != 0u;
            const unsigned bits = __float_as_uint(x);
            ubits[n] = (allowed && x > 0.0f && bits >= tau) ? bits : 0u;
            udoc[n] = (int)(a.doc_base + doc);
        }
        topk_fold<IVFPQ_NPT, true>(ubits, udoc, a.k, M.tk, M.hist);
    }
    __syncthreads();
    topk_shrink(a.k, M.tk, M.hist);
    const unsigned cnt = M.tk.count;
    const int64_t o = p * a.k;
    for (unsigned i = tid; i < cnt; i += THREADS) {
        a.cand_doc[o + i] = M.tk.doc[i];
        a.cand_score[o + i] = __uint_as_float(M.tk.bits[i]);
    }
    if (tid == 0) a.cand_count[p] = (int)cnt;
}

// ================================================================================================ scorer of given docs
struct IvfpqDocsArgs {
    const pq_v4u *codes;
    const float *cb, *queries;
    const int32_t *doc_row, *tile_list, *cand_doc, *cand_count;
    int32_t *cand_list;  // [nq][m]: the candidate's list, -1 where it scores +0.0f
    float *out_score;    // in: the coarse terms; out: the scores
    int64_t n_docs, doc_base, n_tiles, ldq;
    int dim, M, np, m, nlist;
};
// the packed row of candidate c of query q, or -1
__device__ __forceinline__ int64_t ivfpq_cand_row(const IvfpqDocsArgs &a, int q, int64_t c, int64_t lim) {
    if (c >= lim) return -1;
    const int64_t local = (int64_t)gload_i32(a.cand_doc + (int64_t)q * a.m + c) - a.doc_base;
    if (local < 0 || local >= a.n_docs) return -1;
    const int64_t row = gload_i32(a.doc_row + local);
    return row >= 0 && row < a.n_tiles * 64 ? row : -1;
}
__device__ __forceinline__ int64_t ivfpq_cand_lim(const IvfpqDocsArgs &a, int q) {
    int64_t lim = a.m;
    if (a.cand_count != nullptr) lim = min(lim, (int64_t)max(gload_i32(a.cand_count + q), 0));
    return lim;
}
__global__ __launch_bounds__(THREADS) void srx_ivfpq_cand_lists_kernel(IvfpqDocsArgs a) {
    const int q = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (c >= a.m) return;
    const int64_t row = ivfpq_cand_row(a, q, c, ivfpq_cand_lim(a, q));
    int list = -1;
    if (row >= 0) {
        list = gload_i32(a.tile_list + (row >> 6));
        if (list < 0 || list >= a.nlist) list = -1;
    }
    a.cand_list[(int64_t)q * a.m + c] = list;
}
template <int DSUB>
__global__ __launch_bounds__(IVFPQ_DOCS_THREADS) void srx_ivfpq_score_docs_kernel(IvfpqDocsArgs a) {
    __shared__ float lut[IVFPQ_MAX_M * 256];
    const int tid = threadIdx.x, q = blockIdx.x;
    const float *qrow = a.queries + (int64_t)q * a.ldq;
    for (int i = tid; i < a.M * 256; i += IVFPQ_DOCS_THREADS) {  // srx_pq_lut's rule, straight into LDS
        const int m = i >> 8;
        const hf_v4f *cw = reinterpret_cast<const hf_v4f *>(a.cb + (int64_t)i * DSUB);
        float s = 0.0f;
#pragma unroll
        for (int j4 = 0; j4 < DSUB / 4; ++j4) {
            const hf_v4f v = cw[j4];
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int col = m * DSUB + 4 * j4 + u;
                const float qv = col < a.dim ? qrow[col] : 0.0f;
                s = s + qv * e[u];
            }
        }
        lut[i] = s;
    }
    __syncthreads();
    const int64_t lim = ivfpq_cand_lim(a, q);
    for (int64_t c = (int64_t)blockIdx.y * IVFPQ_DOCS_THREADS + tid; c < a.m; c += (int64_t)gridDim.y * IVFPQ_DOCS_THREADS) {
        const int64_t at = (int64_t)q * a.m + c;
        float res = 0.0f;
        if (gload_i32(a.cand_list + at) >= 0) {  // a list: the row is a packed row
            const int64_t row = ivfpq_cand_row(a, q, c, lim);
            const pq_v4u *prow = a.codes + ((row >> 6) * a.np) * 64 + (row & 63);  // + 64 per piece
            float acc = 0.0f;
            for (int p = 0; p < a.np; ++p) {
                const pq_v4u piece = prow[(int64_t)p * 64];
#pragma unroll
                for (int b = 0; b < 16; ++b)
                    if (16 * p + b < a.M) acc = acc + lut[(16 * p + b) * 256 + pq_byte(piece, b)];  // the search's chain
            }
            res = a.out_score[at] + acc;  // fl(coarse + s)
        }
        a.out_score[at] = res;
    }
}

// ================================================================================================ host side
// the geometry of a call: dsub in {4, 8, 16}, 1 <= dim <= 1024, M = ceil(dim / dsub) <= 128, dim_pad = dim rounded up to 64
int ivfpq_geometry(const char *who, int32_t type, int32_t dim, int32_t dsub, int32_t dim_pad, int32_t nlist, int *M) {
    if (!type_ok(type)) return fail(SRX_ERR_INVALID, "%s: type must be SRX_HALF_F16 or SRX_HALF_BF16", who);
    if (dsub != 4 && dsub != 8 && dsub != 16) return fail(SRX_ERR_INVALID, "%s: dsub must be 4, 8 or 16", who);
    if (dim < 1 || dim > 1024) return fail(SRX_ERR_INVALID, "%s: need 1 <= dim <= 1024", who);
    *M = (dim + dsub - 1) / dsub;
    if (*M > IVFPQ_MAX_M) return fail(SRX_ERR_INVALID, "%s: M = ceil(dim / dsub) must be <= 128", who);
    if (dim_pad != (dim + 63) / 64 * 64) return fail(SRX_ERR_INVALID, "%s: dim_pad must be dim rounded up to a multiple of 64", who);
    if (nlist < 1 || nlist > IVFPQ_MAX_LIST) return fail(SRX_ERR_INVALID, "%s: need 1 <= nlist <= 65536", who);
    return SRX_OK;
}

struct IvfpqPlan {
    int64_t ldc, L;  // the centroid score row; tiles a slice holds at most
    int P, S;        // queries per pass, slices per query
};
inline IvfpqPlan ivfpq_plan(int nq, int nlist, int nprobe, int64_t max_list_tiles) {
    IvfpqPlan p;
    p.ldc = (int64_t)((nlist + 31) / 32) * 32;
    const int64_t T = (int64_t)nprobe * max_list_tiles;
    int64_t qb = (1ll << 30) / (256 * T);
    qb = qb < 1 ? 1 : qb > IVFPQ_PASS ? IVFPQ_PASS : qb;
    p.P = (int)(nq < qb ? nq : qb);
    int64_t s = 512 / (p.P > 0 ? p.P : 1);
    if (s > 64) s = 64;
    if (s > (T + 15) / 16) s = (T + 15) / 16;
    p.S = (int)(s < 1 ? 1 : s);
    p.L = (T + p.S - 1) / p.S;
    return p;
}
struct IvfpqWs {
    float *cscores, *lut, *probe_score, *coarse, *strips;
    int32_t *probe_list, *tstart, *pre, *strip_tile;
    srx_rows cand;
    void *merge;
    int64_t merge_bytes, bytes;
};
inline IvfpqWs ivfpq_ws(void *base, const IvfpqPlan &pl, int nprobe, int k, int M) {
    IvfpqWs w;
    char *p = (char *)base;
    auto take = [&](int64_t bytes) {
        char *r = p;
        p += r256(bytes);
        return r;
    };
    const int64_t N = (int64_t)pl.P * nprobe, items = (int64_t)pl.P * pl.S;
    w.cscores = (float *)take(pl.P * pl.ldc * 4);
    w.lut = (float *)take((int64_t)pl.P * M * 1024);
    w.probe_list = (int32_t *)take(N * 4);
    w.probe_score = (float *)take(N * 4);
    w.tstart = (int32_t *)take(N * 4);
    w.coarse = (float *)take(N * 4);
    w.pre = (int32_t *)take((int64_t)pl.P * (nprobe + 1) * 4);
    w.strips = (float *)take(items * pl.L * 256);
    w.strip_tile = (int32_t *)take(items * pl.L * 4);
    int32_t *cd = (int32_t *)take(items * k * 4);
    float *cs = (float *)take(items * k * 4);
    w.cand = srx_plain_rows(cd, cs, (int32_t *)take(items * 4), k);
    w.merge_bytes = srx_merge_workspace_bytes(pl.P, pl.S, k);
    w.merge = p;
    p += w.merge_bytes;
    w.bytes = (int64_t)(p - (char *)base) + 256;
    return w;
}

int check_desc(const char *who, const srx_ivfpq_desc *d, int32_t nq, const float *queries, int *M) {
    if (d == nullptr) return fail(SRX_ERR_INVALID, "%s: null desc", who);
    const int rc = ivfpq_geometry(who, d->type, d->dim, d->dsub, d->dim_pad, d->nlist, M);
    if (rc != SRX_OK) return rc;
    if (d->n_docs < 1 || d->n_docs > SRX_FILTER_MAX_DOCS) return fail(SRX_ERR_INVALID, "%s: n_docs out of range", who);
    if (d->nlist > d->n_docs) return fail(SRX_ERR_INVALID, "%s: need 1 <= nlist <= min(n_docs, 65536)", who);
    if (d->n_tiles < 1 || d->n_tiles > IVFPQ_MAX_TILES) return fail(SRX_ERR_INVALID, "%s: n_tiles out of range", who);
    if (d->max_list_tiles < 1 || d->max_list_tiles > d->n_tiles) return fail(SRX_ERR_INVALID, "%s: need 1 <= max_list_tiles <= n_tiles", who);
    if (d->doc_base < 0 || d->doc_base + d->n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: doc_base + n_docs must fit int32", who);
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if (nq > 0) {
        if (!d->codes || !d->codebooks || !d->centroids || !d->list_tile || !d->row_doc || !d->doc_row || !d->tile_list)
            return fail(SRX_ERR_INVALID, "%s: desc holds a null pointer", who);
        if (!queries) return fail(SRX_ERR_INVALID, "%s: null queries", who);
        if (((uintptr_t)d->codes | (uintptr_t)d->codebooks | (uintptr_t)d->centroids) & 15)
            return fail(SRX_ERR_INVALID, "%s: codes / codebooks / centroids must be 16-byte aligned", who);
        if ((uintptr_t)queries & 15) return fail(SRX_ERR_INVALID, "%s: queries must be 16-byte aligned", who);
    }
    return SRX_OK;
}

template <int TYPE>
void ivfpq_launch_encode(const IvfpqEncodeArgs &a, int dsub, hipStream_t stream) {
    const dim3 grid((unsigned)((a.tiles * IVFPQ_TILE + THREADS - 1) / THREADS), (unsigned)a.np);
    switch (dsub) {
    case 4: hipLaunchKernelGGL((srx_ivfpq_encode_kernel<4, TYPE>), grid, dim3(THREADS), 0, stream, a); break;
    case 8: hipLaunchKernelGGL((srx_ivfpq_encode_kernel<8, TYPE>), grid, dim3(THREADS), 0, stream, a); break;
    default: hipLaunchKernelGGL((srx_ivfpq_encode_kernel<16, TYPE>), grid, dim3(THREADS), 0, stream, a); break;
    }
}
void ivfpq_launch_scan(const IvfpqScanArgs &a, int items, hipStream_t stream) {
    const dim3 grid((unsigned)items);
#define SRX_IVFPQ(NP) \
    case NP: hipLaunchKernelGGL(srx_ivfpq_scan_kernel<NP>, grid, dim3(ivfpq_scan_threads(NP)), 0, stream, a); break;
    switch (ivfpq_pieces(a.M)) { SRX_IVFPQ(1) SRX_IVFPQ(2) SRX_IVFPQ(3) SRX_IVFPQ(4) SRX_IVFPQ(5) SRX_IVFPQ(6) SRX_IVFPQ(7) SRX_IVFPQ(8) }
#undef SRX_IVFPQ
}

}  // namespace

SRX_API int srx_ivfpq_encode(int32_t device, int32_t type, const void *centroids_packed, int32_t nlist, int32_t dim_pad, const float *x, int64_t ld,
                             int64_t n_src, int32_t dim, int32_t dsub, const float *codebooks, const int32_t *src_row, const int32_t *row_list,
                             int64_t n_rows, int64_t row0, int64_t n_total, void *out_codes, void *stream_v) {
    const char *who = "srx_ivfpq_encode";
    int M = 0;
    const int rc = ivfpq_geometry(who, type, dim, dsub, dim_pad, nlist, &M);
    if (rc != SRX_OK) return rc;
    if (n_src < 0 || n_rows < 0 || row0 < 0 || n_total < 0) return fail(SRX_ERR_INVALID, "%s: negative count", who);
    if (row0 > n_total || n_rows > n_total - row0) return fail(SRX_ERR_INVALID, "%s: row0 + n_rows > n_total", who);
    if (ld < dim) return fail(SRX_ERR_INVALID, "%s: need ld >= dim", who);
    if ((row0 & 63) != 0) return fail(SRX_ERR_INVALID, "%s: row0 must be a multiple of 64", who);
    if (n_rows > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: too many rows in one call", who);
    if (n_rows == 0) return SRX_OK;
    if (!centroids_packed || !x || !codebooks || !src_row || !row_list || !out_codes) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)x & 3) return fail(SRX_ERR_INVALID, "%s: input must be 4-byte aligned", who);
    if (((uintptr_t)centroids_packed | (uintptr_t)codebooks | (uintptr_t)out_codes) & 15)
        return fail(SRX_ERR_INVALID, "%s: centroids / codebooks / out_codes must be 16-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    const IvfpqEncodeArgs a = {x, codebooks, (const unsigned short *)centroids_packed, src_row, row_list, ld, n_src, n_rows, row0 >> 6,
                               (n_rows + IVFPQ_TILE - 1) / IVFPQ_TILE, dim, M, ivfpq_pieces(M), dim_pad / 16, nlist, (pq_v4u *)out_codes};
    if (type == SRX_HALF_F16)
        ivfpq_launch_encode<SRX_HALF_F16>(a, dsub, (hipStream_t)stream_v);
    else
        ivfpq_launch_encode<SRX_HALF_BF16>(a, dsub, (hipStream_t)stream_v);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int64_t srx_ivfpq_workspace_bytes(int32_t nq, int32_t nlist, int32_t nprobe, int32_t k, int32_t M, int64_t max_list_tiles) {
    if (nq < 0 || nlist < 1 || nlist > IVFPQ_MAX_LIST || nprobe < 1 || nprobe > nlist || nprobe > IVFPQ_MAX_PROBE || k < 1 || k > KMAX || M < 1 ||
        M > IVFPQ_MAX_M || max_list_tiles < 1 || max_list_tiles > IVFPQ_MAX_TILES || (int64_t)nprobe * max_list_tiles > IVFPQ_MAX_QUERY_TILES)
        return fail(SRX_ERR_INVALID, "srx_ivfpq_workspace_bytes: bad argument%s");
    return ivfpq_ws(nullptr, ivfpq_plan(nq, nlist, nprobe, max_list_tiles), nprobe, k, M).bytes;
}

SRX_API int srx_ivfpq_search(const srx_ivfpq_desc *desc, const float *queries, int32_t nq, int32_t nprobe, int32_t k, const int32_t *probe_list,
                             const srx_doc_filter *filter, int32_t *out_doc, float *out_score, int32_t *out_count, void *workspace,
                             int64_t workspace_bytes, void *stream_v, float score_offset) {
    const char *who = "srx_ivfpq_search";
    int M = 0;
    int rc = check_desc(who, desc, nq, queries, &M);
    if (rc != SRX_OK) return rc;
    const srx_ivfpq_desc &d = *desc;
    if (nprobe < 1 || nprobe > d.nlist || nprobe > IVFPQ_MAX_PROBE) return fail(SRX_ERR_INVALID, "%s: need 1 <= nprobe <= min(nlist, 1024)", who);
    if (filter != nullptr) {
        rc = srx_check_filter(who, filter);
        if (rc != SRX_OK) return rc;
    }
    if (k < 1 || k > KMAX) return fail(SRX_ERR_INVALID, "%s: need 1 <= k <= 1024", who);
    if ((int64_t)nprobe * d.max_list_tiles > IVFPQ_MAX_QUERY_TILES) return fail(SRX_ERR_INVALID, "%s: nprobe * max_list_tiles must be <= 2^26", who);
    if (nq == 0) return SRX_OK;
    if (!out_doc || !out_score || !out_count) return fail(SRX_ERR_INVALID, "%s: null output", who);
    const IvfpqPlan pl = ivfpq_plan(nq, d.nlist, nprobe, d.max_list_tiles);
    const IvfpqWs w = ivfpq_ws(workspace, pl, nprobe, k, M);
    if (!workspace || workspace_bytes < w.bytes) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = (hipStream_t)stream_v;
    for (int q0 = 0; q0 < nq; q0 += pl.P) {
        const int qb = nq - q0 < pl.P ? nq - q0 : pl.P;
        const float *qsrc = queries + (int64_t)q0 * d.dim_pad;
        // every centroid's score is wanted even for a caller's probe list: the coarse terms
        rc = srx_ivf_probe_pass(d.centroids, d.nlist, d.type, d.dim_pad, qsrc, qb, nprobe, w.probe_list, w.probe_score, w.cscores, pl.ldc, stream);
        if (rc != SRX_OK) return rc;
        rc = srx_pq_lut(d.device, d.codebooks, d.dim, d.dsub, qsrc, d.dim_pad, qb, w.lut, stream_v);
        if (rc != SRX_OK) return rc;
        const IvfpqPrepArgs pa = {probe_list != nullptr ? probe_list + (int64_t)q0 * nprobe : w.probe_list, d.list_tile, w.cscores, w.tstart, w.coarse,
                                  w.pre, pl.ldc, d.n_tiles, d.max_list_tiles, nprobe, d.nlist};
        hipLaunchKernelGGL(srx_ivfpq_prepare_kernel, dim3((unsigned)qb), dim3(THREADS), 0, stream, pa);
        const int items = qb * pl.S;  // <= 1024 * 64
        const IvfpqScanArgs sa = {(const pq_v4u *)d.codes, w.lut, w.pre, w.tstart, w.coarse, w.strips, w.strip_tile, pl.L, M, nprobe, pl.S};
        ivfpq_launch_scan(sa, items, stream);
        const IvfpqRankArgs ra = {w.strips, w.strip_tile, w.pre, d.row_doc, filter ? filter->bits : nullptr, filter ? filter->q_filter : nullptr,
                                  w.cand.doc, w.cand.score, w.cand.count, pl.L, d.n_docs, d.doc_base, srx_filter_row_words(d.n_docs), nprobe, pl.S, k,
                                  q0, score_offset};
        hipLaunchKernelGGL(srx_ivfpq_rank_kernel, dim3((unsigned)items), dim3(THREADS), 0, stream, ra);
        HIP_TRY(hipGetLastError());
        const srx_rows out = srx_plain_rows(out_doc + (int64_t)q0 * k, out_score + (int64_t)q0 * k, out_count + q0, k);
        rc = srx_merge_impl(d.device, w.cand, qb, pl.S, k, 0, out, w.merge, w.merge_bytes, stream_v);
        if (rc != SRX_OK) return rc;
    }
    return SRX_OK;
}

SRX_API int64_t srx_ivfpq_score_docs_workspace_bytes(int32_t nq, int32_t m) {
    if (nq < 0 || m < 1 || (int64_t)nq * (int64_t)m > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "srx_ivfpq_score_docs_workspace_bytes: bad argument%s");
    return r256((int64_t)nq * m * 4) + 256;
}

SRX_API int srx_ivfpq_score_docs(const srx_ivfpq_desc *desc, const float *queries, int32_t nq, const int32_t *cand_doc, const int32_t *cand_count,
                                 int32_t m, float *out_score, void *workspace, int64_t workspace_bytes, void *stream_v) {
    const char *who = "srx_ivfpq_score_docs";
    int M = 0;
    int rc = check_desc(who, desc, nq, queries, &M);
    if (rc != SRX_OK) return rc;
    if (m < 1) return fail(SRX_ERR_INVALID, "%s: m must be >= 1", who);
    if ((int64_t)nq * (int64_t)m > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: nq * m must fit int32", who);
    if (nq == 0) return SRX_OK;
    if (!cand_doc || !out_score) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (!workspace || workspace_bytes < r256((int64_t)nq * m * 4) + 256) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    const srx_ivfpq_desc &d = *desc;
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = (hipStream_t)stream_v;
    const IvfpqDocsArgs a = {(const pq_v4u *)d.codes, d.codebooks, queries, d.doc_row, d.tile_list, cand_doc, cand_count, (int32_t *)workspace, out_score,
                             d.n_docs, d.doc_base, d.n_tiles, d.dim_pad, d.dim, M, ivfpq_pieces(M), m, d.nlist};
    for (int q0 = 0; q0 < nq; q0 += 32768) {  // gridDim.y <= 65535
        IvfpqDocsArgs b = a;
        b.cand_doc += (int64_t)q0 * m;
        if (b.cand_count != nullptr) b.cand_count += q0;
        b.cand_list += (int64_t)q0 * m;
        const int qb = nq - q0 < 32768 ? nq - q0 : 32768;
        hipLaunchKernelGGL(srx_ivfpq_cand_lists_kernel, dim3((unsigned)(((int64_t)m + THREADS - 1) / THREADS), (unsigned)qb), dim3(THREADS), 0, stream, b);
    }
    HIP_TRY(hipGetLastError());
    // the coarse terms: the candidates' lists as rows of the centroid corpus (-1 and entries behind the count give +0.0f)
    rc = srx_dense_score_docs_half(d.device, d.type, d.centroids, d.nlist, d.dim_pad, queries, nq, 0, a.cand_list, cand_count, m, out_score, stream_v);
    if (rc != SRX_OK) return rc;
    const int64_t chunks = ((int64_t)m + IVFPQ_DOCS_CHUNK - 1) / IVFPQ_DOCS_CHUNK;
    const dim3 grid((unsigned)nq, (unsigned)(chunks < 64 ? chunks : 64));
    switch (d.dsub) {
    case 4: hipLaunchKernelGGL(srx_ivfpq_score_docs_kernel<4>, grid, dim3(IVFPQ_DOCS_THREADS), 0, stream, a); break;
    case 8: hipLaunchKernelGGL(srx_ivfpq_score_docs_kernel<8>, grid, dim3(IVFPQ_DOCS_THREADS), 0, stream, a); break;
    default: hipLaunchKernelGGL(srx_ivfpq_score_docs_kernel<16>, grid, dim3(IVFPQ_DOCS_THREADS), 0, stream, a); break;
    }
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
