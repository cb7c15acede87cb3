// dense_mx.hip -- the MX dense index (include/mx/sparse_rx_mx.h): MXFP8 / MXFP4 rows with one e8m0 scale per 32 columns, kept in
// the operand order of v_mfma_scale_f32_32x32x64_f8f6f4, the quantiser that writes them, two score kernels, the ranking and the
// scorer of given docs.  Replaces nothing in the reference project: it has no such index.
//
//   convert   one workgroup per tile of 32 rows, one wave per row at a time, a lane four columns per 256: the row is read once
//             (16-byte loads when base, ld and dim allow), a block's amax is the maximum over its 8 lanes (three xor shuffles),
//             a non-finite row is found by a ballot and zeroed.  Codes and scale bytes go to the tile's image in LDS and leave
//             it as contiguous fragment-ordered pieces and scale dwords.  The SAME kernel packs a pass's queries as MXFP8 into
//             the workspace: the A operand has the order of an FP8 corpus.
//   stream    nq <= 32, memory-bound: the one query tile and its scale dwords sit in LDS; every wave walks its own doc tiles
//             (tile = wave, wave + n_waves, ...) and loads a group of up to four k-steps of a tile straight from memory into
//             registers -- the corpus is in fragment order, a wave's load of a (tile, k-step) is one contiguous 2 KiB or 1 KiB --
//             with the next group's loads issued before this group's MFMAs (two register sets, the waits counted by the
//             compiler).  No corpus byte passes through LDS.
//   GEMM      nq > 32, compute-bound: a workgroup = 128 queries x 128 docs, four waves 2 x 2, a wave 2 x 2 tiles; one k-step (64
//             columns) per stage, both operands staged through LDS in two buffers as two planes of 16 bytes per lane (a wave's
//             ds_read_b128 is a contiguous KiB), the next stage's global loads in flight over the MFMAs, one barrier per stage;
//             a wave's scale dwords come from memory once per four k-steps.
//   Both kernels: every output element is ONE chain of the instruction over s = 0, 1, ... ascending from +0.0f, each k-step
//   with its own scale bytes (op_sel = s & 3 of the lane's dword).  Scores go to the [queries][ld] fp32 matrix of the pass.
//   rank      the half index's fold (optional filter row, offset applied) on topk_fold / topk_shrink, then srx_merge_impl.
//   scorer    one wave per (query, 32 candidates): the candidates' pieces and scale dwords gathered as B, the query quantised
//             by the lane into every row of A, the same chain; row 0 of the result is read.
#include "half_common.h"  // the pass plan and the workspace of a search are the half index's
#include "mx/sparse_rx_mx.h"

namespace {

typedef int mx_v8i __attribute__((ext_vector_type(8)));

// ================================================================================================ formats and the quantiser
template <int TYPE> struct MxFmt;
template <> struct MxFmt<SRX_MX_FP8> {  // e4m3
    static constexpr int EMAX = 8, EMIN = -6, MBITS = 3, SIGN = 0x80, BLGP = 0, PIECE16 = 2;  // PIECE16: 16-byte units per piece
    static constexpr float MAXV = 448.0f;
};
template <> struct MxFmt<SRX_MX_FP4> {  // e2m1
    static constexpr int EMAX = 2, EMIN = 0, MBITS = 1, SIGN = 0x8, BLGP = 4, PIECE16 = 1;
    static constexpr float MAXV = 6.0f;
};
inline int mx_sg(int ks) { return (ks + 3) / 4; }
inline int64_t mx_code_bytes(int type, int64_t tiles, int dim_pad) { return tiles * 32 * (int64_t)dim_pad / (type == SRX_MX_FP8 ? 1 : 2); }

// the block exponent e of a block whose largest |x| has the bits `amax` (finite): e + 127 is the scale code
template <int TYPE>
__device__ __forceinline__ int mx_block_exp(unsigned amax) {
    if (amax == 0u) return 0;
    return max((int)(amax >> 23) - 127 - MxFmt<TYPE>::EMAX, -127);  // <= 127 - EMAX: the upper clamp never binds
}
// 2^(-e): -e is in [EMAX - 127, 127], a normal f32
__device__ __forceinline__ float mx_inv_scale(int e) { return __uint_as_float((unsigned)(127 - e) << 23); }
// x * mult -> the element code.  The product is exact unless it falls below 2^-126, and then it is below half the smallest
// element (2^-10, 2^-2) and rounds to zero as the exact value does.  The clamp is plain arithmetic; rintf rounds to nearest
// even, and an even n is an even code.
template <int TYPE>
__device__ __forceinline__ unsigned mx_quant(float x, float mult) {
    typedef MxFmt<TYPE> F;
    const float v = x * mult;
    const float a = fminf(fabsf(v), F::MAXV);
    const int ec = max((int)(__float_as_uint(a) >> 23) - 127, F::EMIN);  // the exponent of the quantum's binade
    const float t = a * __uint_as_float((unsigned)(127 + F::MBITS - ec) << 23);  // in [0, 2^(MBITS + 1)]: exact
    const unsigned q = ((unsigned)(ec - F::EMIN) << F::MBITS) + (unsigned)(int)rintf(t);
    return (q != 0u && v < 0.0f) ? (q | (unsigned)F::SIGN) : q;
}
__device__ __forceinline__ bool mx_nonfinite(float x) { return (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u; }

// ================================================================================================ convert (and query pack)
constexpr int MC_TILE = 32;               // rows per workgroup
constexpr int MC_ROWS = MC_TILE / WAVES;  // rows per wave

struct MxConvertArgs {
    const float *in;      // the chunk's rows (row stride ld elements)
    int64_t ld, n_rows;   // rows of this call
    int64_t tile0;        // the chunk's first tile in the whole corpus
    int dim, dim_pad;
    hf_v4i *codes;        // the WHOLE corpus' codes
    uint32_t *scales;     // ... and scale dwords
    int32_t *flag;        // may be null
};

template <int NJ, bool VEC, int TYPE>
__global__ __launch_bounds__(THREADS) void srx_mx_convert_kernel(MxConvertArgs a) {
    typedef MxFmt<TYPE> F;
    constexpr int ROWB = TYPE == SRX_MX_FP8 ? NJ * 256 : NJ * 128;  // code bytes of a row of the image
    constexpr int PITCH = ROWB + 16;
    __shared__ __attribute__((aligned(16))) unsigned char tile[MC_TILE * PITCH];
    __shared__ unsigned char sc[MC_TILE * 32];  // [row][block of 32 columns]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * MC_TILE;            // the tile's first row, relative to the chunk
    const int live = (int)min((int64_t)MC_TILE, a.n_rows - t0);  // rows of the tile this call holds (>= 1)
    bool flagged = false;                                        // wave-uniform
    for (int g = 0; g < MC_ROWS; ++g) {
        const int r = wave * MC_ROWS + g;
        const float *row = a.in + (t0 + r) * a.ld;
        float x[NJ][4];
        unsigned amax[NJ];
        bool bad = false;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = 4 * lane + 256 * j;
#pragma unroll
            for (int e = 0; e < 4; ++e) x[j][e] = 0.0f;  // columns past dim and rows the call does not hold: zeros
            if (r < live) {
                if constexpr (VEC) {  // dim % 4 == 0: the four columns are inside the row together
                    if (c < a.dim) {
                        const hf_v4f v = *reinterpret_cast<const hf_v4f *>(row + c);
                        x[j][0] = v.x; x[j][1] = v.y; x[j][2] = v.z; x[j][3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < a.dim) x[j][e] = row[c + e];
                }
            }
            unsigned m = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                bad = bad || mx_nonfinite(x[j][e]);
                m = max(m, __float_as_uint(x[j][e]) & 0x7FFFFFFFu);  // |x| of finite values orders as its bits do
            }
#pragma unroll
            for (int d = 1; d < 8; d <<= 1) m = max(m, (unsigned)__shfl_xor((int)m, d));  // the block's 8 lanes
            amax[j] = m;
        }
        bad = __ballot(bad) != 0ull;  // the whole row is the wave's
        flagged = flagged || bad;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = 4 * lane + 256 * j;
            const int e = bad ? 0 : mx_block_exp<TYPE>(amax[j]);
            const float mult = mx_inv_scale(e);
            unsigned q[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) q[i] = bad ? 0u : mx_quant<TYPE>(x[j][i], mult);
            if constexpr (TYPE == SRX_MX_FP8)
                *reinterpret_cast<unsigned *>(tile + r * PITCH + c) = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
            else
                *reinterpret_cast<unsigned short *>(tile + r * PITCH + (c >> 1)) = (unsigned short)(q[0] | (q[1] << 4) | (q[2] << 8) | (q[3] << 12));
            if ((lane & 7) == 0) sc[r * 32 + (c >> 5)] = (unsigned char)(e + 127);  // c >> 5 < 8 NJ <= 32
        }
    }
    if (flagged && lane == 0 && a.flag != nullptr) atomicOr(a.flag, SRX_QUANT_NONFINITE);
    __syncthreads();
    const int ks = a.dim_pad >> 6, sg = (ks + 3) >> 2;
    const int64_t t = a.tile0 + blockIdx.x;
    // 16-byte unit i of the tile's codes: piece i / PIECE16 = (k-step, lane), lane = row (l & 31), half l >> 5 (the header's order)
    const int units = ks * 64 * F::PIECE16;
    for (int i = threadIdx.x; i < units; i += THREADS) {
        const int piece = i / F::PIECE16, part = i % F::PIECE16, s = piece >> 6, l = piece & 63;
        const int byte = TYPE == SRX_MX_FP8 ? 64 * s + 32 * part + 16 * (l >> 5) : 32 * s + 16 * (l >> 5);  // FP8: 16 columns of each block
        a.codes[t * units + i] = *reinterpret_cast<const hf_v4i *>(tile + (l & 31) * PITCH + byte);
    }
    for (int i = threadIdx.x; i < sg * 64; i += THREADS) {
        const int gq = i >> 6, l = i & 63;
        unsigned w = 0u;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int s = 4 * gq + u;
            w |= (s < ks ? (unsigned)sc[(l & 31) * 32 + 2 * s + (l >> 5)] : 127u) << (8 * u);
        }
        a.scales[t * (sg * 64) + i] = w;
    }
}

template <int TYPE>
void mc_launch(const MxConvertArgs &a, bool vec, hipStream_t stream) {
    const unsigned blocks = (unsigned)((a.n_rows + MC_TILE - 1) / MC_TILE);
    const int nj = (a.dim_pad + 255) / 256;
#define SRX_MC(NJ)                                                                                                          \
    if (nj == NJ) {                                                                                                         \
        if (vec)                                                                                                            \
            hipLaunchKernelGGL((srx_mx_convert_kernel<NJ, true, TYPE>), dim3(blocks), dim3(THREADS), 0, stream, a);         \
        else                                                                                                                \
            hipLaunchKernelGGL((srx_mx_convert_kernel<NJ, false, TYPE>), dim3(blocks), dim3(THREADS), 0, stream, a);        \
        return;                                                                                                             \
    }
    SRX_MC(1) SRX_MC(2) SRX_MC(3) SRX_MC(4)
#undef SRX_MC
}

// ================================================================================================ the instruction
// acc += A (32 queries x 64, FP8) * B (64 x 32 docs, TYPE), the lane's 32 elements of each scaled by byte OP of its dword
template <int TYPE, int OPA, int OPB>
__device__ __forceinline__ hf_v16f mx_mfma(const mx_v8i &a, const mx_v8i &b, const hf_v16f &acc, unsigned sa, unsigned sb) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, acc, 0, MxFmt<TYPE>::BLGP, OPA, (int)sa, OPB, (int)sb);
}
__device__ __forceinline__ mx_v8i mx_join(const hf_v4i &lo, const hf_v4i &hi) { return (mx_v8i){lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w}; }
// D[row = query][col = doc]: lane l holds doc l & 31, queries (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)
__device__ __forceinline__ void mx_store_tile(const hf_v16f &acc, int64_t q0, int64_t d, int h, int nq, int64_t n_docs, float *scores, int64_t ld) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int64_t q = q0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        if (q < nq && d < n_docs) scores[q * ld + d] = acc[reg];
    }
}

// ================================================================================================ stream (nq <= 32)
struct MxScoreArgs {
    const hf_v4i *codes;     // corpus
    const uint32_t *scales;
    const hf_v4i *qcodes;    // the pass's queries, MXFP8 in fragment order
    const uint32_t *qscales;
    float *scores;
    int64_t n_docs, n_tiles, ld;
    int ks, sg, nq, n_qtiles;
};
constexpr int MS_MAX_BLOCKS = 1024;  // four workgroups per compute unit: each wave then walks its tiles with two groups in flight

template <int TYPE>
struct MxGroup {  // the B operand of up to four k-steps of one tile, and their scale dword
    hf_v4i lo[4], hi[4];
    unsigned sc;
};

template <int TYPE>
__global__ __launch_bounds__(THREADS) void srx_mx_stream_scores_kernel(MxScoreArgs a) {
    __shared__ hf_v4i qa[16 * 128];  // [k-step][16-byte half][lane]: 32 KiB at dim_pad 1024
    __shared__ unsigned qs[4 * 64];  // [group of four k-steps][lane]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    for (int i = threadIdx.x; i < a.ks * 128; i += THREADS) qa[(i >> 7) * 128 + (i & 1) * 64 + ((i >> 1) & 63)] = a.qcodes[i];
    for (int i = threadIdx.x; i < a.sg * 64; i += THREADS) qs[i] = a.qscales[i];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * WAVES;
    auto load = [&](MxGroup<TYPE> &b, int64_t t, int g) __attribute__((always_inline)) {
        b.sc = a.scales[(t * a.sg + g) * 64 + lane];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int s = 4 * g + u;
            if (s < a.ks) {  // uniform
                const int64_t piece = (t * a.ks + s) * 64 + lane;
                if constexpr (TYPE == SRX_MX_FP8) {
                    b.lo[u] = a.codes[2 * piece];
                    b.hi[u] = a.codes[2 * piece + 1];
                } else {
                    b.lo[u] = a.codes[piece];
                }
            }
        }
    };
    hf_v16f acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    int64_t t = (int64_t)blockIdx.x * WAVES + wave;
    int g = 0;
    // one step: issue the next group's loads, then this group's chain links (ascending k), then the tile's store
    auto step = [&](MxGroup<TYPE> &cur, MxGroup<TYPE> &nxt) __attribute__((always_inline)) {
        const bool last = g + 1 == a.sg;
        const int64_t nt = last ? t + stride : t;
        const int ng = last ? 0 : g + 1;
        if (nt < a.n_tiles) load(nxt, nt, ng);
        const unsigned sa = qs[g * 64 + lane];
#define SRX_MX_LINK(U)                                                                                                  \
        if (4 * g + U < a.ks) {                                                                                         \
            const int s = 4 * g + U;                                                                                    \
            const mx_v8i A = mx_join(qa[s * 128 + lane], qa[s * 128 + 64 + lane]);                                      \
            const mx_v8i B = mx_join(cur.lo[U], TYPE == SRX_MX_FP8 ? cur.hi[U] : (hf_v4i){0, 0, 0, 0});                 \
            acc = mx_mfma<TYPE, U, U>(A, B, acc, sa, cur.sc);                                                           \
        }
        SRX_MX_LINK(0) SRX_MX_LINK(1) SRX_MX_LINK(2) SRX_MX_LINK(3)
#undef SRX_MX_LINK
        if (last) {
            mx_store_tile(acc, 0, t * 32 + r, h, a.nq, a.n_docs, a.scores, a.ld);
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        }
        t = nt;
        g = ng;
    };
    MxGroup<TYPE> b0, b1;
    if (t < a.n_tiles) load(b0, t, 0);
    while (t < a.n_tiles) {
        step(b0, b1);
        if (t >= a.n_tiles) break;
        step(b1, b0);
    }
}

// ================================================================================================ GEMM (nq > 32)
// Workgroup b serves query block b % n_qblocks and doc block b / n_qblocks: the workgroups that read one block of docs run together.
template <int TYPE>
__global__ __launch_bounds__(THREADS) void srx_mx_gemm_scores_kernel(MxScoreArgs a, int n_qblocks) {
    constexpr int BU = 64 * MxFmt<TYPE>::PIECE16;  // 16-byte units of a doc tile's k-step
    constexpr int BL = 4 * BU / THREADS;           // ... a thread moves per stage: 2 (FP8) or 1 (FP4)
    __shared__ hf_v4i sA[2][4][128];               // [buffer][query tile][16-byte half][lane]
    __shared__ hf_v4i sB[2][4][BU];                // [buffer][doc tile][16-byte half][lane]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int qblock = (int)(blockIdx.x % (unsigned)n_qblocks);
    const int64_t dblock = blockIdx.x / (unsigned)n_qblocks;
    const int64_t qt0 = (int64_t)qblock * 4, dt0 = dblock * 4;  // first tiles of 32
    const int wq = wave >> 1, wd = wave & 1;                    // the wave's 64 queries and 64 docs of the block
    hf_v4i ga[2], gb[BL];
    // unit x = tid + 256 j of an operand's four tiles: tile x / units-per-tile, unit u of the piece order -> plane (u & 1), lane u >> 1
    auto load_stage = [&](int s) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int x = tid + THREADS * j, ti = x >> 7;
            ga[j] = (hf_v4i){0, 0, 0, 0};
            if (qt0 + ti < a.n_qtiles) ga[j] = a.qcodes[((qt0 + ti) * a.ks + s) * 128 + (x & 127)];
        }
#pragma unroll
        for (int j = 0; j < BL; ++j) {
            const int x = tid + THREADS * j, ti = x / BU;
            gb[j] = (hf_v4i){0, 0, 0, 0};
            if (dt0 + ti < a.n_tiles) gb[j] = a.codes[((dt0 + ti) * a.ks + s) * BU + (x % BU)];
        }
    };
    auto store_stage = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int x = tid + THREADS * j, u = x & 127;
            sA[buf][x >> 7][(u & 1) * 64 + (u >> 1)] = ga[j];
        }
#pragma unroll
        for (int j = 0; j < BL; ++j) {
            const int x = tid + THREADS * j, u = x % BU;
            if constexpr (TYPE == SRX_MX_FP8)
                sB[buf][x / BU][(u & 1) * 64 + (u >> 1)] = gb[j];
            else
                sB[buf][x / BU][u] = gb[j];
        }
    };
    hf_v16f acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    load_stage(0);
    store_stage(0);
    __syncthreads();
    for (int g = 0; g < a.sg; ++g) {
        unsigned sa[2], sb[2];  // the scale dwords of this group of k-steps; a tile that does not exist: 2^0 on zero codes
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t qt = qt0 + 2 * wq + i, dt = dt0 + 2 * wd + i;
            sa[i] = qt < a.n_qtiles ? a.qscales[(qt * a.sg + g) * 64 + lane] : 0x7F7F7F7Fu;
            sb[i] = dt < a.n_tiles ? a.scales[(dt * a.sg + g) * 64 + lane] : 0x7F7F7F7Fu;
        }
#define SRX_MX_STAGE(U)                                                                                                 \
        if (4 * g + U < a.ks) { /* uniform; the buffer of k-step 4 g + U is U & 1 */                                   \
            const bool more = 4 * g + U + 1 < a.ks;                                                                     \
            if (more) load_stage(4 * g + U + 1); /* in flight over this stage's MFMAs */                                \
            mx_v8i A[2], B[2];                                                                                          \
            _Pragma("unroll") for (int i = 0; i < 2; ++i) {                                                             \
                A[i] = mx_join(sA[U & 1][2 * wq + i][lane], sA[U & 1][2 * wq + i][64 + lane]);                          \
                if constexpr (TYPE == SRX_MX_FP8)                                                                       \
                    B[i] = mx_join(sB[U & 1][2 * wd + i][lane], sB[U & 1][2 * wd + i][BU - 64 + lane]);                 \
                else                                                                                                    \
                    B[i] = mx_join(sB[U & 1][2 * wd + i][lane], (hf_v4i){0, 0, 0, 0});                                  \
            }                                                                                                           \
            _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                               \
                _Pragma("unroll") for (int j = 0; j < 2; ++j) acc[i][j] = mx_mfma<TYPE, U, U>(A[i], B[j], acc[i][j], sa[i], sb[j]); \
            if (more) store_stage((U & 1) ^ 1); /* that buffer was last read one barrier ago */                         \
            __syncthreads();                                                                                            \
        }
        SRX_MX_STAGE(0) SRX_MX_STAGE(1) SRX_MX_STAGE(2) SRX_MX_STAGE(3)
#undef SRX_MX_STAGE
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
            mx_store_tile(acc[i][j], (qt0 + 2 * wq + i) * 32, (dt0 + 2 * wd + j) * 32 + r, h, a.nq, a.n_docs, a.scores, a.ld);
}

// ================================================================================================ rank
// srx_dense_half_topk_kernel's semantics: one workgroup per (query, split of the columns) folds its slice of the score row into
// an exact lazy top-k list; the ranked value of column c is fl32(score + offset), a result iff > 0 and (with a filter row) bit
// c of the row is set.
__global__ __launch_bounds__(THREADS) void srx_mx_topk_kernel(const float *__restrict__ scores, int64_t ld, int64_t n_docs, int nq, int k,
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
constexpr int MD_CHUNK = 32;  // candidates per wave: the columns of one MFMA tile
struct MxDocsArgs {
    const hf_v4i *codes;
    const uint32_t *scales;
    const float *queries;
    const int32_t *cand_doc, *cand_count;
    float *out_score;
    int64_t n_docs, doc_base, waves;  // waves = nq * chunks
    int ks, sg, m, chunks;
};
template <int TYPE>
__global__ __launch_bounds__(THREADS) void srx_mx_score_docs_kernel(MxDocsArgs a) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t w = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w >= a.waves) return;  // whole waves leave
    const int q = (int)(w / a.chunks);
    const int64_t c = (w - (int64_t)q * a.chunks) * MD_CHUNK + r;  // both halves of the wave hold candidate r's row
    int64_t lim = a.m;
    if (a.cand_count != nullptr) lim = min(lim, (int64_t)max(gload_i32(a.cand_count + q), 0));
    int row = -1;  // padding, outside the corpus, beyond m
    if (c < lim) {
        const int64_t local = (int64_t)gload_i32(a.cand_doc + (int64_t)q * a.m + c) - a.doc_base;
        if (local >= 0 && local < a.n_docs) row = (int)local;  // n_docs < 2^31
    }
    float res = 0.0f;
    if (__ballot(row >= 0) != 0ull) {  // uniform
        const float *qrow = a.queries + (int64_t)q * (a.ks * 64);
        bool bad = false;  // a non-finite query is zeros, as the search's pack makes it
        for (int cc = 4 * lane; cc < a.ks * 64; cc += 256) {
            const hf_v4f v = *reinterpret_cast<const hf_v4f *>(qrow + cc);
            bad = bad || mx_nonfinite(v.x) || mx_nonfinite(v.y) || mx_nonfinite(v.z) || mx_nonfinite(v.w);
        }
        bad = __ballot(bad) != 0ull;
        const int64_t t = (row >= 0 ? row : 0) >> 5;
        const int bl = ((row >= 0 ? row : 0) & 31) + 32 * h;  // the lane of the candidate's pieces
        hf_v16f acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        for (int g = 0; g < a.sg; ++g) {  // the search's chain: ascending k from +0.0f; the query is every row of A
            const unsigned sb = row >= 0 ? a.scales[(t * a.sg + g) * 64 + bl] : 0x7F7F7F7Fu;
#define SRX_MX_LINK(U)                                                                                                  \
            if (4 * g + U < a.ks) { /* uniform */                                                                       \
                const int s = 4 * g + U;                                                                                \
                hf_v4i blo = {0, 0, 0, 0}, bhi = {0, 0, 0, 0};                                                          \
                if (row >= 0) {                                                                                         \
                    const int64_t piece = (t * a.ks + s) * 64 + bl;                                                     \
                    if constexpr (TYPE == SRX_MX_FP8) {                                                                 \
                        blo = a.codes[2 * piece];                                                                       \
                        bhi = a.codes[2 * piece + 1];                                                                   \
                    } else {                                                                                            \
                        blo = a.codes[piece];                                                                           \
                    }                                                                                                   \
                }                                                                                                       \
                /* the lane owns the scale of block h of the k-step (columns 64 s + 32 h .. + 31: x) and holds 16 columns of  \
                   each block, 32 b + 16 h .. + 15: those of its own block are x[4 h ..], those of the other block y */     \
                const hf_v4f *src = reinterpret_cast<const hf_v4f *>(qrow + 64 * s + 32 * h);                           \
                const hf_v4f *oth = reinterpret_cast<const hf_v4f *>(qrow + 64 * s + 32 * (1 - h) + 16 * h);            \
                hf_v4f x[8], y[4];                                                                                      \
                unsigned am = 0u;                                                                                       \
                _Pragma("unroll") for (int i = 0; i < 8; ++i) {                                                         \
                    x[i] = src[i];                                                                                      \
                    _Pragma("unroll") for (int e = 0; e < 4; ++e) am = max(am, __float_as_uint(x[i][e]) & 0x7FFFFFFFu); \
                }                                                                                                       \
                _Pragma("unroll") for (int i = 0; i < 4; ++i) y[i] = oth[i];                                            \
                const int ex = bad ? 0 : mx_block_exp<SRX_MX_FP8>(am);                                                  \
                const int exo = __shfl_xor(ex, 32); /* the other block's, from the lane that owns it */                  \
                const float m0 = mx_inv_scale(h ? exo : ex), m1 = mx_inv_scale(h ? ex : exo);                           \
                mx_v8i A;                                                                                               \
                _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                         \
                    const hf_v4f v0 = h ? y[i] : x[i], v1 = h ? x[4 + i] : y[i];                                        \
                    unsigned w0 = 0u, w1 = 0u;                                                                          \
                    _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                     \
                        w0 |= (bad ? 0u : mx_quant<SRX_MX_FP8>(v0[e], m0)) << (8 * e);                                  \
                        w1 |= (bad ? 0u : mx_quant<SRX_MX_FP8>(v1[e], m1)) << (8 * e);                                  \
                    }                                                                                                   \
                    A[i] = (int)w0;                                                                                     \
                    A[4 + i] = (int)w1;                                                                                 \
                }                                                                                                       \
                acc = mx_mfma<TYPE, 0, U>(A, mx_join(blo, bhi), acc, (unsigned)(ex + 127), sb);                         \
            }
            SRX_MX_LINK(0) SRX_MX_LINK(1) SRX_MX_LINK(2) SRX_MX_LINK(3)
#undef SRX_MX_LINK
        }
        if (row >= 0) res = acc[0];  // lanes 0 .. 31, register 0: row 0 of the tile, column = candidate r
    }
    if (h == 0 && c < a.m) a.out_score[(int64_t)q * a.m + c] = res;
}

// ================================================================================================ host side
bool type_ok(int32_t type) { return type == SRX_MX_FP8 || type == SRX_MX_FP4; }
const char *TYPE_MSG = "%s: type must be SRX_MX_FP8 or SRX_MX_FP4";
uint32_t *mx_scales_of(const void *buf, int type, int64_t n_rows, int dim_pad) {
    return (uint32_t *)((char *)buf + mx_code_bytes(type, hf_tiles(n_rows), dim_pad));
}

}  // namespace

SRX_API int64_t srx_mx_bytes(int32_t type, int64_t n_rows, int32_t dim_pad) {
    if (!type_ok(type) || n_rows < 0 || !hf_dim_ok(dim_pad))
        return fail(SRX_ERR_INVALID, "srx_mx_bytes: need a type of srx_mx_type, n_rows >= 0 and dim_pad a multiple of 64, <= 1024%s");
    return mx_code_bytes(type, hf_tiles(n_rows), dim_pad) + hf_tiles(n_rows) * mx_sg(dim_pad / 64) * 256;
}

SRX_API int srx_mx_convert(int32_t device, int32_t type, const float *emb, int64_t ld, int64_t n_rows, int32_t dim, int32_t dim_pad, int64_t row0,
                           int64_t n_total, void *out, int32_t *flag, void *stream_v) {
    const char *who = "srx_mx_convert";
    if (!type_ok(type)) return fail(SRX_ERR_INVALID, TYPE_MSG, who);
    if (n_rows < 0 || row0 < 0 || n_total < 0) return fail(SRX_ERR_INVALID, "%s: negative count", who);
    if (row0 > n_total || n_rows > n_total - row0) return fail(SRX_ERR_INVALID, "%s: row0 + n_rows > n_total", who);
    if (!hf_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: unsupported dim_pad (a multiple of 64, <= 1024)", who);
    if (dim < 1 || dim > dim_pad || ld < dim) return fail(SRX_ERR_INVALID, "%s: need 1 <= dim <= dim_pad and ld >= dim", who);
    if ((row0 & 31) != 0) return fail(SRX_ERR_INVALID, "%s: row0 must be a multiple of 32", who);
    if ((n_rows + MC_TILE - 1) / MC_TILE > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: too many rows in one call", who);
    if (n_rows == 0) return SRX_OK;
    if (!emb || !out) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)emb & 3) return fail(SRX_ERR_INVALID, "%s: input must be 4-byte aligned", who);
    if ((uintptr_t)out & 15) return fail(SRX_ERR_INVALID, "%s: out must be 16-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    const MxConvertArgs a = {emb, ld, n_rows, row0 >> 5, dim, dim_pad, (hf_v4i *)out, mx_scales_of(out, type, n_total, dim_pad), flag};
    const bool vec = ((uintptr_t)emb & 15) == 0 && ld % 4 == 0 && dim % 4 == 0;
    if (type == SRX_MX_FP8)
        mc_launch<SRX_MX_FP8>(a, vec, (hipStream_t)stream_v);
    else
        mc_launch<SRX_MX_FP4>(a, vec, (hipStream_t)stream_v);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int64_t srx_mx_workspace_bytes(int32_t nq, int64_t n_docs, int32_t k) {
    if (nq < 0 || n_docs <= 0 || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "srx_mx_workspace_bytes: bad argument%s");
    return half_ws(nullptr, half_plan(nq, n_docs, k), k).bytes;  // its query block (2 KiB per query) holds 1024 codes + 32 scale bytes
}

SRX_API int srx_mx_search(int32_t device, int32_t type, const void *corpus, int64_t n_docs, int32_t dim_pad, const float *queries, int32_t nq,
                          int32_t k, int64_t doc_base, const srx_doc_filter *filter, int32_t *out_doc, float *out_score, int32_t *out_count,
                          void *workspace, int64_t workspace_bytes, void *stream_v, float score_offset) {
    const char *who = "srx_mx_search";
    if (!type_ok(type)) return fail(SRX_ERR_INVALID, TYPE_MSG, who);
    if (filter != nullptr) {
        const int rc = srx_check_filter(who, filter);
        if (rc != SRX_OK) return rc;
    }
    if (nq < 0 || n_docs <= 0 || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "%s: need n_docs > 0, 1 <= k <= 1024", who);
    if (!hf_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 64, <= 1024 (pad the rows with zeros)", who);
    if (doc_base < 0 || doc_base + n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: doc_base + n_docs must fit int32", who);
    if (nq == 0) return SRX_OK;
    if (!corpus || !queries || !out_doc || !out_score || !out_count) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)corpus | (uintptr_t)queries) & 15) return fail(SRX_ERR_INVALID, "%s: corpus / queries must be 16-byte aligned", who);
    const HalfPlan p = half_plan(nq, n_docs, k);
    const HalfWs w = half_ws(workspace, p, k);
    if (!workspace || workspace_bytes < w.bytes) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    const int ks = dim_pad / 64;
    const uint32_t *fbits = filter ? filter->bits : nullptr;
    const int32_t *qf = filter ? filter->q_filter : nullptr;
    for (int q0 = 0; q0 < nq; q0 += p.QB) {
        const int qb = nq - q0 < p.QB ? nq - q0 : p.QB;
        // the pass's queries as an MXFP8 "corpus" of qb rows in the workspace: the A operand
        uint32_t *qscales = mx_scales_of(w.qpack, SRX_MX_FP8, qb, dim_pad);
        const MxConvertArgs pack = {queries + (int64_t)q0 * dim_pad, dim_pad, qb, 0, dim_pad, dim_pad, w.qpack, qscales, nullptr};
        mc_launch<SRX_MX_FP8>(pack, true, stream);
        const MxScoreArgs a = {(const hf_v4i *)corpus, mx_scales_of(corpus, type, n_docs, dim_pad), w.qpack, qscales, w.scores,
                               n_docs, hf_tiles(n_docs), p.ld, ks, mx_sg(ks), qb, (int)hf_tiles(qb)};
        if (qb <= 32) {
            const int64_t want = (a.n_tiles + WAVES - 1) / WAVES;
            const dim3 grid((unsigned)(want < MS_MAX_BLOCKS ? want : MS_MAX_BLOCKS));
            if (type == SRX_MX_FP8)
                hipLaunchKernelGGL(srx_mx_stream_scores_kernel<SRX_MX_FP8>, grid, dim3(THREADS), 0, stream, a);
            else
                hipLaunchKernelGGL(srx_mx_stream_scores_kernel<SRX_MX_FP4>, grid, dim3(THREADS), 0, stream, a);
        } else {
            const int n_qblocks = (qb + HF_QTILE - 1) / HF_QTILE;
            const dim3 grid((unsigned)((n_docs + HF_QTILE - 1) / HF_QTILE * n_qblocks));  // <= 2^24 * 8
            if (type == SRX_MX_FP8)
                hipLaunchKernelGGL(srx_mx_gemm_scores_kernel<SRX_MX_FP8>, grid, dim3(THREADS), 0, stream, a, n_qblocks);
            else
                hipLaunchKernelGGL(srx_mx_gemm_scores_kernel<SRX_MX_FP4>, grid, dim3(THREADS), 0, stream, a, n_qblocks);
        }
        hipLaunchKernelGGL(srx_mx_topk_kernel, dim3((unsigned)((int64_t)qb * p.ns)), dim3(THREADS), 0, stream, (const float *)w.scores, p.ld, n_docs, qb,
                           (int)k, p.ns, doc_base, score_offset, fbits, srx_filter_row_words(n_docs), qf, q0, w.cand.doc, w.cand.score, w.cand.count);
        HIP_TRY(hipGetLastError());
        const srx_rows out = srx_plain_rows(out_doc + (int64_t)q0 * k, out_score + (int64_t)q0 * k, out_count + q0, k);
        const int rc = srx_merge_impl(device, w.cand, qb, p.ns, k, 0, out, nullptr, 0, stream_v);
        if (rc != SRX_OK) return rc;
    }
    return SRX_OK;
}

SRX_API int srx_mx_score_docs(int32_t device, int32_t type, const void *corpus, int64_t n_docs, int32_t dim_pad, const float *queries, int32_t nq,
                              int64_t doc_base, const int32_t *cand_doc, const int32_t *cand_count, int32_t m, float *out_score, void *stream_v) {
    const char *who = "srx_mx_score_docs";
    if (!type_ok(type)) return fail(SRX_ERR_INVALID, TYPE_MSG, who);
    if (!hf_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 64, <= 1024 (pad the rows with zeros)", who);
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if (m < 1) return fail(SRX_ERR_INVALID, "%s: m must be >= 1", who);
    if ((int64_t)nq * (int64_t)m > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: nq * m must fit int32", who);
    if (n_docs <= 0 || n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: n_docs out of range", who);
    if (doc_base < 0) return fail(SRX_ERR_INVALID, "%s: doc_base < 0", who);
    if (nq == 0) return SRX_OK;
    if (!corpus || !queries || !cand_doc || !out_score) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)corpus | (uintptr_t)queries) & 15) return fail(SRX_ERR_INVALID, "%s: corpus / queries must be 16-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    const int chunks = (int)(((int64_t)m + MD_CHUNK - 1) / MD_CHUNK), ks = dim_pad / 64;
    const MxDocsArgs a = {(const hf_v4i *)corpus, mx_scales_of(corpus, type, n_docs, dim_pad), queries, cand_doc, cand_count, out_score,
                          n_docs, doc_base, (int64_t)nq * chunks, ks, mx_sg(ks), m, chunks};
    const dim3 grid((unsigned)((a.waves + WAVES - 1) / WAVES));  // waves <= nq * m < 2^31
    if (type == SRX_MX_FP8)
        hipLaunchKernelGGL(srx_mx_score_docs_kernel<SRX_MX_FP8>, grid, dim3(THREADS), 0, (hipStream_t)stream_v, a);
    else
        hipLaunchKernelGGL(srx_mx_score_docs_kernel<SRX_MX_FP4>, grid, dim3(THREADS), 0, (hipStream_t)stream_v, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
