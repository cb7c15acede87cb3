// dense_binary_asym.hip -- asymmetric scores over the binary dense index (include/asym/sparse_rx_binary_asym.h): the corpus is the
// tiled 1-bit buffer of dense_binary.hip as it is, the query keeps a 4-bit code per dimension, and the score
// s = sum code * (2 bit - 1) is an integer.  Replaces nothing in the reference project: it has no binary index.
//
// A translation unit of its own (as dense_binary.hip is): one more user of topk_fold / topk_shrink, and inside another file that
// would change what the compiler inlines into the kernels already there.
//
//   quantise  one wave per query, a lane per 16 columns: a wave max of |q - center|, then 16 codes per lane, one 16-byte store.
//   prep      one wave per query of the pass, a lane per 16 codes: the sum of the codes, and either (bit-plane route) the four
//             plane words per 32 dimensions of u = code + 8, or (MFMA route) the 16-byte piece stored where the score kernel reads
//             its A operands.
//   planes    few queries.  The shape of srx_binary_dist_kernel: a wave owns a 64-row tile, a lane keeps its doc's W words and
//             their popcount in VGPRs, a query's plane words are wave-uniform scalar loads.  Per 32 dimensions and (doc, query):
//             four v_and_b32 with a scalar operand and four accumulating v_bcnt_u32_b32, one chain per plane; then
//             t = sum_j 2^j popc(d & P_j) - 8 popc(d) and s = 2 t - qsum.
//   mfma      batches.  A workgroup of eight waves stages the codes of 128 queries in LDS once, in A-operand order, and every
//             wave walks 64-row doc tiles: it loads the tile's 16-byte pieces as the Hamming kernel does, makes lanes l and l + 32
//             hold two words of the SAME doc with v_permlane32_swap_b32 (no trip through LDS), expands 4 bits to four 0/1 bytes
//             at a time in registers and issues v_mfma_i32_32x32x32_i8 against the four 32-query A operands with the same
//             expanded B: the expansion is paid once per (doc tile, query tile).  s = 2 acc - qsum.
//
//             The k positions: the instruction sums over 32 positions, lane (n, h) of an operand feeding positions 16 h .. 16 h + 15
//             of row / column n (dense.hip).  For the word pair p (words 2 p and 2 p + 1 of a row) and t in {0, 1}, MFMA step
//             2 p + t puts COLUMN 64 p + 32 h + 16 t + i at position 16 h + i: after the swap lane (n, h) holds word 2 p + h of doc n,
//             and step t expands its bits 16 t .. 16 t + 15, byte i from bit i -- four v_bfe / v_mul / v_and triples, no shuffles
//             of bytes.  A is read with the same map, and there it is free: 16 consecutive codes of a row are one 16-byte piece.
//             Because the sum is an integer sum, any permutation the two operands share gives the same word.
//
//             128 queries per tile, not 64: 128 * dim_pad <= 128 KiB fits gfx950's 160 KiB at every dim_pad, and the ~13 VALU
//             instructions that expand 16 bits are then shared by four MFMAs (64 cycles each) instead of two.  The eight waves are
//             two per SIMD, so one wave's expansion and epilogue run under the other's MFMAs; above 512 dimensions that is one
//             workgroup per CU, and what a second resident workgroup would hide is already hidden by the second wave.  A wave
//             takes the two 32-doc halves of its tile one after the other: 64 accumulator registers, not 128, which keeps every
//             instance within the 256 registers that two waves per SIMD leave; an A operand is read from LDS once per half.
//   rank      srx_binary_topk_kernel's fold loop over a row of the u16 matrix.  The entry is a = s + 7 dim_pad + 1 in
//             [1, 14 337]: exact in fp32, ordered as s, and 0xFFFF stays free for "not a candidate".  Then srx_merge_impl, then
//             a back to s.
//   given     a wave per (query, 64 candidates): a lane gathers its doc's pieces from the tiled layout; the plane words of 64
//             dimensions at a time come from four ballots over the query's codes, so there is no workspace.
#include "filter_common.h"
#include "asym/sparse_rx_binary_asym.h"

namespace {

typedef unsigned ba_v4u __attribute__((ext_vector_type(4)));
typedef unsigned ba_v2u __attribute__((ext_vector_type(2)));
typedef int ba_v4i __attribute__((ext_vector_type(4)));
typedef int ba_v16i __attribute__((ext_vector_type(16)));

constexpr int BA_TILE = 64;        // rows per tile of the corpus: one per lane
constexpr int BA_QTILE = 128;      // queries per workgroup of either score kernel
constexpr int BA_PASS = 1024;      // queries per pass at most
constexpr int BA_NPT = 16;         // columns per thread and step of the rank kernel
constexpr int BA_SPLIT_DOCS = THREADS * BA_NPT * 4;  // a row split is at least this many docs
constexpr int BA_MWAVES = 8;       // waves of an MFMA workgroup: two per SIMD
constexpr int BA_MTHREADS = BA_MWAVES * 64;
constexpr int BA_MAX_TPW = 8;      // doc tiles one wave of the MFMA kernel walks at most
constexpr unsigned BA_NONE = 0xFFFFu;  // matrix entry of a lane that is not a candidate
constexpr int BA_MIN = (int)0x80000000;  // the score of padding

inline bool ba_dim_ok(int dim_pad) { return dim_pad >= 128 && dim_pad <= 1024 && dim_pad % 128 == 0; }
inline int64_t ba_tiles(int64_t n_rows) { return (n_rows + BA_TILE - 1) / BA_TILE; }

__device__ __forceinline__ int ba_byte(unsigned w, int i) { return (int)(w << (24 - 8 * i)) >> 24; }  // signed byte i of a word
__device__ __forceinline__ int ba_sum16(const ba_v4u &p) {
    int s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) s += ba_byte(p.x, i) + ba_byte(p.y, i) + ba_byte(p.z, i) + ba_byte(p.w, i);
    return s;
}

// ================================================================================================ quantise
__global__ __launch_bounds__(THREADS) void srx_binary_asym_quantize_kernel(const float *__restrict__ q, int64_t ld, int nq, int dim, int dim_pad,
                                                                            const float *__restrict__ center, ba_v4u *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (row >= nq) return;  // whole waves leave
    const float *x = q + (int64_t)row * ld;
    const int c0 = 16 * lane;
    float r[16];
    unsigned mx = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int c = c0 + i;
        r[i] = 0.0f;
        if (c < dim) r[i] = center != nullptr ? x[c] - center[c] : x[c];
        const float v = fabsf(r[i]);
        if (v == v) mx = max(mx, __float_as_uint(v));  // the bits of non-negative floats order as the floats do
    }
    const float amax = __uint_as_float(wave_max(mx));
    const float inv = amax > 0.0f ? 7.0f / amax : 0.0f;
    unsigned w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float p = r[i] * inv;
        int code = 0;
        if (p == p) code = (int)fminf(fmaxf(rintf(p), -7.0f), 7.0f);
        if (c0 + i >= dim) code = 0;
        w[i >> 2] |= ((unsigned)code & 0xFFu) << (8 * (i & 3));
    }
    if (c0 < dim_pad) out[((int64_t)row * dim_pad + c0) >> 4] = (ba_v4u){w[0], w[1], w[2], w[3]};
}

// ================================================================================================ prep of a pass
// planes: u32[nq][W][4], word j of (q, w) has bit c = bit j of code[q][32 w + c] + 8.  apack: the A operands, 16 bytes at
// ((q >> 5) * W + 2 p + t) * 64 + (q & 31) + 32 h for the piece at column 64 p + 32 h + 16 t; the rows q >= nq of the last 32: zeros.
template <bool MFMA>
__global__ __launch_bounds__(THREADS) void srx_binary_asym_prep_kernel(const ba_v4u *__restrict__ codes, int nq, int nq32, int W,
                                                                        ba_v4u *__restrict__ out, int32_t *__restrict__ qsum) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (q >= (MFMA ? nq32 : nq)) return;  // whole waves leave
    ba_v4u p = {0, 0, 0, 0};
    const bool piece = lane < 2 * W;  // lane i: the codes of columns 16 i .. 16 i + 15
    if (piece && q < nq) p = codes[(int64_t)q * 2 * W + lane];
    const int total = (int)wave_sum((unsigned)ba_sum16(p));
    if (lane == 0) qsum[q] = total;
    if constexpr (MFMA) {
        const int pr = lane >> 2, h = (lane >> 1) & 1, t = lane & 1;
        if (piece) out[((int64_t)(q >> 5) * W + 2 * pr + t) * 64 + (q & 31) + 32 * h] = p;
    } else {
        const unsigned wd[4] = {p.x, p.y, p.z, p.w};
        unsigned pl[4] = {0, 0, 0, 0};  // 16 bits of each plane
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const unsigned u = (unsigned)(ba_byte(wd[i >> 2], i & 3) + 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) pl[j] |= ((u >> j) & 1u) << i;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) pl[j] |= (unsigned)__shfl_down((int)pl[j], 1) << 16;  // the even lane takes the odd lane's half
        if (piece && (lane & 1) == 0) out[(int64_t)q * W + (lane >> 1)] = (ba_v4u){pl[0], pl[1], pl[2], pl[3]};
    }
}

// ================================================================================================ the scores of a pass
struct BaScoreArgs {
    const ba_v4u *corpus;
    const void *prep;     // the pass's planes or A operands
    const int32_t *qsum;  // the pass's code sums
    int64_t n_docs, ld, n_tiles;
    int nq, n_qtiles, bias, tpw;  // bias = 7 dim_pad + 1; tpw: tiles per wave (MFMA)
    const uint32_t *filter_bits;  // null: no filter
    int64_t filter_words;
    const int32_t *q_filter;  // the pass's entries (null: row 0)
    uint16_t *mat;            // [nq][ld]
};

// NJ = W / 4 pieces per doc.  Workgroup b serves query tile b % n_qtiles of tile group b / n_qtiles.
template <int NJ>
__global__ __launch_bounds__(THREADS) void srx_binary_asym_plane_kernel(BaScoreArgs a) {
    constexpr int W = 4 * NJ;
    const int lane = threadIdx.x & 63;
    const int qt = (int)(blockIdx.x % (unsigned)a.n_qtiles);
    const int64_t tile = (int64_t)(blockIdx.x / (unsigned)a.n_qtiles) * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (tile >= a.n_tiles) return;  // whole waves leave
    const int64_t d = tile * BA_TILE + lane;
    unsigned x[W];
    int popd = 0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {  // rows past n_docs in the last tile exist in the buffer (zeros)
        const ba_v4u p = a.corpus[(tile * NJ + j) * 64 + lane];
        x[4 * j] = p.x;
        x[4 * j + 1] = p.y;
        x[4 * j + 2] = p.z;
        x[4 * j + 3] = p.w;
        popd += __builtin_popcount(p.x) + __builtin_popcount(p.y) + __builtin_popcount(p.z) + __builtin_popcount(p.w);
    }
    const bool inside = d < a.n_docs;
    const int q_end = min(a.nq, (qt + 1) * BA_QTILE);
    for (int q = qt * BA_QTILE; q < q_end; ++q) {  // uniform
        const SRX_CONSTANT uint32_t *pw = (const SRX_CONSTANT uint32_t *)((const uint32_t *)a.prep + (int64_t)q * W * 4);
        unsigned a0 = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) {
            a0 += (unsigned)__builtin_popcount(x[w] & pw[4 * w]);
            a1 += (unsigned)__builtin_popcount(x[w] & pw[4 * w + 1]);
            a2 += (unsigned)__builtin_popcount(x[w] & pw[4 * w + 2]);
            a3 += (unsigned)__builtin_popcount(x[w] & pw[4 * w + 3]);
        }
        const int t = (int)(a0 + 2 * a1 + 4 * a2 + 8 * a3) - 8 * popd;
        const int s = 2 * t - cload_i32(a.qsum + q);
        bool allowed = inside;
        if (a.filter_bits != nullptr) {
            const int fr = a.q_filter != nullptr ? cload_i32(a.q_filter + q) : 0;
            if (fr >= 0) {  // uniform; the tile's two words: inside the row (its length is a multiple of 4 words)
                const SRX_CONSTANT uint32_t *frow = (const SRX_CONSTANT uint32_t *)(a.filter_bits + (int64_t)fr * a.filter_words + 2 * tile);
                const unsigned long long mask = (unsigned long long)frow[0] | ((unsigned long long)frow[1] << 32);
                allowed = allowed && ((mask >> lane) & 1ull) != 0ull;
            }
        }
        a.mat[(int64_t)q * a.ld + d] = (uint16_t)(allowed ? (unsigned)(s + a.bias) : BA_NONE);  // d < ld
    }
}

// bits 0 .. 15 of x -> 16 bytes of 0 / 1, byte i from bit i: a nibble times (1 + 2^7 + 2^14 + 2^21) puts bit k at position 8 k
// (the four shifted copies do not overlap, so nothing carries)
__device__ __forceinline__ ba_v4i ba_expand16(unsigned x) {
    ba_v4i r;
    r.x = (int)(((x & 15u) * 0x00204081u) & 0x01010101u);
    r.y = (int)((((x >> 4) & 15u) * 0x00204081u) & 0x01010101u);
    r.z = (int)((((x >> 8) & 15u) * 0x00204081u) & 0x01010101u);
    r.w = (int)((((x >> 12) & 15u) * 0x00204081u) & 0x01010101u);
    return r;
}

template <int NJ>
__global__ __launch_bounds__(BA_MTHREADS) void srx_binary_asym_mfma_kernel(BaScoreArgs a) {
    constexpr int W = 4 * NJ;
    extern __shared__ __attribute__((aligned(16))) unsigned char ba_lds[];
    ba_v4i *sA = (ba_v4i *)ba_lds;                      // [4 groups of 32 queries][W steps][64 lanes]
    int *sQs = (int *)(ba_lds + BA_QTILE * W * 32);     // [128] code sums
    int *sFr = sQs + BA_QTILE;                          // [128] filter rows
    const int tid = threadIdx.x, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qt = (int)(blockIdx.x % (unsigned)a.n_qtiles);
    const int q_lo = qt * BA_QTILE;
    const int ng = min(4, (a.nq - q_lo + 31) / 32);  // 32-query operands of this tile (>= 1)
    {
        const ba_v4i *src = (const ba_v4i *)a.prep + (int64_t)qt * 4 * W * 64;
        for (int i = tid; i < ng * W * 64; i += BA_MTHREADS) sA[i] = src[i];
        if (tid < BA_QTILE) {
            const int q = q_lo + tid;
            sQs[tid] = q < a.nq ? a.qsum[q] : 0;
            sFr[tid] = (q < a.nq && a.q_filter != nullptr) ? a.q_filter[q] : 0;
        }
    }
    __syncthreads();
    const int64_t t0 = ((int64_t)(blockIdx.x / (unsigned)a.n_qtiles) * BA_MWAVES + wave) * a.tpw;
    for (int it = 0; it < a.tpw; ++it) {  // uniform
        const int64_t tile = t0 + it;
        if (tile >= a.n_tiles) break;
        ba_v4u pc[NJ];
#pragma unroll
        for (int j = 0; j < NJ; ++j) pc[j] = a.corpus[(tile * NJ + j) * 64 + lane];  // rows past n_docs exist (zeros)
#pragma unroll 1
        for (int hf = 0; hf < 2; ++hf) {  // the docs 32 hf .. 32 hf + 31 of the tile: 64 accumulator registers at a time
            ba_v16i acc[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = (ba_v16i){0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int p = 0; p < 2 * NJ; ++p) {  // word pair p of the row
                const unsigned w0 = (p & 1) ? pc[p >> 1].z : pc[p >> 1].x, w1 = (p & 1) ? pc[p >> 1].w : pc[p >> 1].y;
                // lanes 32 .. 63 of the first <-> lanes 0 .. 31 of the second: sw.x = (word 2p of doc n, word 2p + 1 of doc n) for the
                // docs 0 .. 31 of the tile, sw.y the same for the docs 32 .. 63
                const ba_v2u sw = __builtin_amdgcn_permlane32_swap(w0, w1, false, false);
                const unsigned word = hf ? sw.y : sw.x;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const ba_v4i b = ba_expand16(word >> (16 * t));
#pragma unroll
                    for (int g = 0; g < 4; ++g)
                        if (g < ng) acc[g] = __builtin_amdgcn_mfma_i32_32x32x32_i8(sA[(g * W + 2 * p + t) * 64 + lane], b, acc[g], 0, 0, 0);  // uniform
                }
            }
            // D[query][doc]: lane (r, h) holds doc r of the half, queries (reg & 3) + 8 (reg >> 2) + 4 h of the operand.  The row part
            // of an address is uniform (a multiple of ld), the lane part one 64-bit value.
            const int64_t d = tile * BA_TILE + 32 * hf + r;
            const bool inside = d < a.n_docs;
            uint16_t *out = a.mat + (int64_t)(q_lo + 4 * h) * a.ld + d;  // d < ld
            const int lim = a.nq - q_lo - 4 * h;                         // rows of this lane below it exist
            const uint32_t *fw = a.filter_bits != nullptr ? a.filter_bits + 2 * tile + hf : nullptr;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                if (g >= ng) continue;  // uniform
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const ba_v4i qs = *(const ba_v4i *)&sQs[32 * g + 8 * k + 4 * h], fr = *(const ba_v4i *)&sFr[32 * g + 8 * k + 4 * h];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = 32 * g + 8 * k + i;  // of the query tile, less 4 h
                        if (row >= lim) continue;
                        const int s = 2 * acc[g][4 * k + i] - qs[i];
                        bool allowed = inside;
                        if (fw != nullptr && fr[i] >= 0) allowed = allowed && ((fw[(int64_t)fr[i] * a.filter_words] >> r) & 1u) != 0u;
                        out[(int64_t)row * a.ld] = (uint16_t)(allowed ? (unsigned)(s + a.bias) : BA_NONE);
                    }
                }
            }
        }
    }
}

// ================================================================================================ rank
// One workgroup per (query, split of the columns) folds its slice of the matrix row into an exact lazy top-m list of
// (a as fp32 bits, doc): srx_binary_topk_kernel with the entry itself as the ranked value.
__global__ __launch_bounds__(THREADS) void srx_binary_asym_topk_kernel(const uint16_t *__restrict__ mat, int64_t ld, int64_t n_docs, int nq, int m,
                                                                       int n_splits, int64_t doc_base, int32_t *__restrict__ cand_doc,
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
    const uint16_t *row = mat + (int64_t)q * ld;
    for (int64_t c0 = lo; c0 < hi; c0 += (int64_t)THREADS * BA_NPT) {
        unsigned ubits[BA_NPT];
        int udoc[BA_NPT];
        const unsigned tau = M.tk.tau;
#pragma unroll
        for (int n = 0; n < BA_NPT; ++n) {
            const int64_t c = c0 + (int64_t)n * THREADS + tid;
            unsigned v = BA_NONE;
            if (c < hi) v = row[c];
            const unsigned b = __float_as_uint((float)v);  // 1 <= v <= 14 337: exact
            ubits[n] = (v != BA_NONE && b >= tau) ? b : 0u;
            udoc[n] = (int)(doc_base + c);
        }
        topk_fold<BA_NPT, true>(ubits, udoc, m, M.tk, M.hist);
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

// the merged rows' values back to scores: entry i of row q is a result iff i < count[q]
__global__ __launch_bounds__(THREADS) void srx_binary_asym_emit_kernel(const float *__restrict__ val, const int32_t *__restrict__ count, int64_t n, int m,
                                                                       int bias, int32_t *__restrict__ out_score) {
    const int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t q = i / m;
    out_score[i] = (int)(i - q * m) < count[q] ? (int)val[i] - bias : BA_MIN;
}

// ================================================================================================ scores of given docs
struct BaDocsArgs {
    const ba_v4u *corpus;
    const int8_t *codes;
    const int32_t *cand_doc, *cand_count;
    int32_t *out_score;
    int64_t n_docs, doc_base, waves;  // waves = nq * chunks
    int nj, m, chunks;
};
__global__ __launch_bounds__(THREADS) void srx_binary_asym_score_docs_kernel(BaDocsArgs a) {
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
    const ba_v4u *prow = a.corpus + ((max(row, (int64_t)0) >> 6) * a.nj) * 64 + (max(row, (int64_t)0) & 63);  // + 64 per piece
    const int8_t *qrow = a.codes + (int64_t)q * a.nj * 128;
    unsigned acc[4] = {0, 0, 0, 0};
    int popd = 0, mine = 0;
    for (int j = 0; j < a.nj; ++j) {  // uniform: every lane of the wave takes part in the ballots
        ba_v4u p = {0, 0, 0, 0};
        if (row >= 0) p = prow[(int64_t)j * 64];
        const unsigned wd[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
        for (int hw = 0; hw < 2; ++hw) {  // 64 columns: lane l holds the code of column 128 j + 64 hw + l
            const int code = qrow[128 * j + 64 * hw + lane];
            mine += code;
            const unsigned u = (unsigned)(code + 8);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const unsigned long long pl = __ballot((u >> k) & 1u);
                acc[k] += (unsigned)(__builtin_popcount(wd[2 * hw] & (unsigned)pl) + __builtin_popcount(wd[2 * hw + 1] & (unsigned)(pl >> 32)));
            }
            popd += __builtin_popcount(wd[2 * hw]) + __builtin_popcount(wd[2 * hw + 1]);
        }
    }
    const int qsum = (int)wave_sum((unsigned)mine);
    const int t = (int)(acc[0] + 2 * acc[1] + 4 * acc[2] + 8 * acc[3]) - 8 * popd;
    if (c < a.m) a.out_score[(int64_t)q * a.m + c] = row >= 0 ? 2 * t - qsum : BA_MIN;
}

// ================================================================================================ host side
// the plan of one search call: query passes and row splits exactly as srx_binary_search makes them
struct BaPlan {
    int QB, qb_max, q32;  // queries per pass; of the largest pass; that rounded up to 32
    int64_t ld;
    int ns;
};
inline BaPlan ba_plan(int nq, int64_t n_docs, int m) {
    BaPlan p;
    p.ld = ba_tiles(n_docs) * BA_TILE;
    const int64_t q = (4ll << 30) / (p.ld * 2) / 32 * 32;
    p.QB = (int)(q < 32 ? 32 : q > BA_PASS ? BA_PASS : q);
    p.qb_max = nq < p.QB ? nq : p.QB;
    p.q32 = (p.qb_max + 31) / 32 * 32;
    int64_t s = 2048 / (p.qb_max > 0 ? p.qb_max : 1);
    const int64_t by_docs = n_docs / BA_SPLIT_DOCS, cap = (MERGE_NPT * THREADS) / (m > 0 ? m : 1);  // one merge level
    if (s > by_docs) s = by_docs;
    if (s > cap) s = cap;
    p.ns = (int)(s < 1 ? 1 : s);
    return p;
}
struct BaWs {
    uint16_t *mat;   // [qb_max][ld]
    srx_rows cand;   // [qb_max * ns] lists of m
    float *val;      // [qb_max][m]: the merged rows' ranked values
    void *prep;      // the pass's planes or A operands
    int32_t *qsum;   // [q32]
    int64_t bytes;
};
inline BaWs ba_ws(void *base, const BaPlan &pl, int m, int dim_pad) {
    BaWs w;
    char *p = (char *)base;
    auto take = [&](int64_t bytes) {
        char *r = p;
        p += (bytes + 255) / 256 * 256;
        return r;
    };
    w.mat = (uint16_t *)take((int64_t)pl.qb_max * pl.ld * 2);
    const int64_t lists = (int64_t)pl.qb_max * pl.ns;
    int32_t *cand_doc = (int32_t *)take(lists * m * 4);
    float *cand_score = (float *)take(lists * m * 4);
    w.cand = srx_plain_rows(cand_doc, cand_score, (int32_t *)take(lists * 4), m);
    w.val = (float *)take((int64_t)pl.qb_max * m * 4);
    w.prep = take((int64_t)pl.q32 * dim_pad);
    w.qsum = (int32_t *)take((int64_t)pl.q32 * 4);
    w.bytes = (int64_t)(p - (char *)base) + 256;
    return w;
}

int ba_launch_planes(const BaScoreArgs &a, int nj, hipStream_t stream) {
    const dim3 grid((unsigned)(((a.n_tiles + WAVES - 1) / WAVES) * a.n_qtiles));  // <= 2^23 * 8
#define SRX_BA(NJ) \
    case NJ: hipLaunchKernelGGL(srx_binary_asym_plane_kernel<NJ>, grid, dim3(THREADS), 0, stream, a); break;
    switch (nj) { SRX_BA(1) SRX_BA(2) SRX_BA(3) SRX_BA(4) SRX_BA(5) SRX_BA(6) SRX_BA(7) SRX_BA(8) }
#undef SRX_BA
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

template <int NJ>
int ba_launch_mfma_nj(const BaScoreArgs &a, const dim3 &grid, hipStream_t stream) {
    const size_t dyn = (size_t)BA_QTILE * NJ * 128 + 2 * BA_QTILE * 4;
    if (dyn > 32768)  // LDS beyond the default limit: opt in (gfx950 has 160 KiB per workgroup)
        HIP_TRY(hipFuncSetAttribute((const void *)srx_binary_asym_mfma_kernel<NJ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    hipLaunchKernelGGL(srx_binary_asym_mfma_kernel<NJ>, grid, dim3(BA_MTHREADS), dyn, stream, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
int ba_launch_mfma(BaScoreArgs a, int nj, hipStream_t stream) {
    // tiles per wave: as many as leave about 2048 workgroups, so the staging of a query tile is shared by more doc tiles
    const int64_t t = a.n_tiles * a.n_qtiles / ((int64_t)BA_MWAVES * 2048);
    a.tpw = (int)(t < 1 ? 1 : t > BA_MAX_TPW ? BA_MAX_TPW : t);
    const int64_t per_wg = (int64_t)BA_MWAVES * a.tpw;
    const dim3 grid((unsigned)(((a.n_tiles + per_wg - 1) / per_wg) * a.n_qtiles));
#define SRX_BA(NJ) \
    case NJ: return ba_launch_mfma_nj<NJ>(a, grid, stream);
    switch (nj) { SRX_BA(1) SRX_BA(2) SRX_BA(3) SRX_BA(4) SRX_BA(5) SRX_BA(6) SRX_BA(7) SRX_BA(8) }
#undef SRX_BA
    return SRX_OK;
}

}  // namespace

SRX_API int srx_binary_asym_quantize(int32_t device, const float *q, int64_t ld, int32_t nq, int32_t dim, int32_t dim_pad, const float *center,
                                     int8_t *out_codes, void *stream_v) {
    const char *who = "srx_binary_asym_quantize";
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if (!ba_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 128, <= 1024", who);
    if (dim < 1 || dim > dim_pad || ld < dim) return fail(SRX_ERR_INVALID, "%s: need 1 <= dim <= dim_pad and ld >= dim", who);
    if (nq == 0) return SRX_OK;
    if (!q || !out_codes) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)q | (uintptr_t)center) & 3) return fail(SRX_ERR_INVALID, "%s: queries and center must be 4-byte aligned", who);
    if ((uintptr_t)out_codes & 15) return fail(SRX_ERR_INVALID, "%s: out_codes must be 16-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(srx_binary_asym_quantize_kernel, dim3((unsigned)((nq + WAVES - 1) / WAVES)), dim3(THREADS), 0, (hipStream_t)stream_v, q, ld,
                       (int)nq, (int)dim, (int)dim_pad, center, (ba_v4u *)out_codes);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int64_t srx_binary_asym_workspace_bytes(int32_t nq, int64_t n_docs, int32_t m, int32_t dim_pad) {
    if (nq < 0 || n_docs <= 0 || m <= 0 || m > KMAX || !ba_dim_ok(dim_pad))
        return fail(SRX_ERR_INVALID, "srx_binary_asym_workspace_bytes: bad argument%s");
    return ba_ws(nullptr, ba_plan(nq, n_docs, m), m, dim_pad).bytes;
}

SRX_API int srx_binary_asym_search(int32_t device, const void *bits_tiled, int64_t n_docs, int32_t dim_pad, const int8_t *q_codes, int32_t nq,
                                   int32_t m, int64_t doc_base, const srx_doc_filter *filter, int32_t *out_doc, int32_t *out_score,
                                   int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream_v, int32_t route) {
    const char *who = "srx_binary_asym_search";
    if (route < 0 || route > 2) return fail(SRX_ERR_INVALID, "%s: route must be 0, 1 or 2", who);
    if (filter != nullptr) {
        const int rc = srx_check_filter(who, filter);
        if (rc != SRX_OK) return rc;
    }
    if (nq < 0 || n_docs <= 0 || m <= 0 || m > KMAX) return fail(SRX_ERR_INVALID, "%s: need n_docs > 0, 1 <= m <= 1024", who);
    if (!ba_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 128, <= 1024", who);
    if (doc_base < 0 || doc_base + n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: doc_base + n_docs must fit int32", who);
    if (nq == 0) return SRX_OK;
    if (!bits_tiled || !q_codes || !out_doc || !out_score || !out_count) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)bits_tiled | (uintptr_t)q_codes) & 15) return fail(SRX_ERR_INVALID, "%s: corpus / q_codes must be 16-byte aligned", who);
    const BaPlan p = ba_plan(nq, n_docs, m);
    const BaWs w = ba_ws(workspace, p, m, dim_pad);
    if (!workspace || workspace_bytes < w.bytes) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    const int W = dim_pad / 32, bias = 7 * dim_pad + 1;
    const bool mfma = route == 2 || (route == 0 && nq >= SRX_BINARY_ASYM_ROUTE_NQ);
    for (int q0 = 0; q0 < nq; q0 += p.QB) {
        const int qb = nq - q0 < p.QB ? nq - q0 : p.QB, qb32 = (qb + 31) / 32 * 32;
        const ba_v4u *codes = (const ba_v4u *)(q_codes + (int64_t)q0 * dim_pad);
        if (mfma)
            hipLaunchKernelGGL(srx_binary_asym_prep_kernel<true>, dim3((unsigned)(qb32 / WAVES)), dim3(THREADS), 0, stream, codes, qb, qb32, W,
                               (ba_v4u *)w.prep, w.qsum);
        else
            hipLaunchKernelGGL(srx_binary_asym_prep_kernel<false>, dim3((unsigned)((qb + WAVES - 1) / WAVES)), dim3(THREADS), 0, stream, codes, qb,
                               qb32, W, (ba_v4u *)w.prep, w.qsum);
        HIP_TRY(hipGetLastError());
        const BaScoreArgs a = {(const ba_v4u *)bits_tiled, w.prep, w.qsum, n_docs, p.ld, ba_tiles(n_docs), qb, (qb + BA_QTILE - 1) / BA_QTILE, bias, 1,
                               filter ? filter->bits : nullptr, srx_filter_row_words(n_docs),
                               filter && filter->q_filter ? filter->q_filter + q0 : nullptr, w.mat};
        int rc = mfma ? ba_launch_mfma(a, W / 4, stream) : ba_launch_planes(a, W / 4, stream);
        if (rc != SRX_OK) return rc;
        hipLaunchKernelGGL(srx_binary_asym_topk_kernel, dim3((unsigned)((int64_t)qb * p.ns)), dim3(THREADS), 0, stream, (const uint16_t *)w.mat, p.ld,
                           n_docs, qb, (int)m, p.ns, doc_base, w.cand.doc, w.cand.score, w.cand.count);
        HIP_TRY(hipGetLastError());
        const srx_rows out = srx_plain_rows(out_doc + (int64_t)q0 * m, w.val, out_count + q0, m);
        rc = srx_merge_impl(device, w.cand, qb, p.ns, m, 0, out, nullptr, 0, stream_v);
        if (rc != SRX_OK) return rc;
        const int64_t n = (int64_t)qb * m;
        hipLaunchKernelGGL(srx_binary_asym_emit_kernel, dim3((unsigned)((n + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, (const float *)w.val,
                           (const int32_t *)(out_count + q0), n, (int)m, bias, out_score + (int64_t)q0 * m);
        HIP_TRY(hipGetLastError());
    }
    return SRX_OK;
}

SRX_API int srx_binary_asym_score_docs(int32_t device, const void *bits_tiled, int64_t n_docs, int32_t dim_pad, const int8_t *q_codes, int32_t nq,
                                       int64_t doc_base, const int32_t *cand_doc, const int32_t *cand_count, int32_t m, int32_t *out_score,
                                       void *stream_v) {
    const char *who = "srx_binary_asym_score_docs";
    if (!ba_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 128, <= 1024", who);
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if (m < 1) return fail(SRX_ERR_INVALID, "%s: m must be >= 1", who);
    if ((int64_t)nq * (int64_t)m > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: nq * m must fit int32", who);
    if (n_docs <= 0 || n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: n_docs out of range", who);
    if (doc_base < 0) return fail(SRX_ERR_INVALID, "%s: doc_base < 0", who);
    if (nq == 0) return SRX_OK;
    if (!bits_tiled || !q_codes || !cand_doc || !out_score) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)bits_tiled | (uintptr_t)q_codes) & 15) return fail(SRX_ERR_INVALID, "%s: corpus / q_codes must be 16-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    const int chunks = (int)(((int64_t)m + 63) / 64);
    const BaDocsArgs a = {(const ba_v4u *)bits_tiled, q_codes, cand_doc, cand_count, out_score, n_docs, doc_base, (int64_t)nq * chunks, dim_pad / 128, m, chunks};
    const dim3 grid((unsigned)((a.waves + WAVES - 1) / WAVES));  // waves <= nq * m < 2^31
    hipLaunchKernelGGL(srx_binary_asym_score_docs_kernel, grid, dim3(THREADS), 0, (hipStream_t)stream_v, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
