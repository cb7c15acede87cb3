// mmr.hip -- diversified top-k (include/sparse_rx_mmr.h): Maximal Marginal Relevance selection over the (doc, score, count)
// lists the searches and the fusion return, with the similarities of the rows of a resident dense index.  Replaces nothing
// in the reference project: it has no diversification.  Same build flags as the other units; -ffp-contract=off is part of
// the contract (every product, sum and difference of the f32 Gram and of the selection is rounded on its own).
//
// Two launches per call, G[nq][m][m] between them in the workspace (or in out_sim):
//   Gram, half  one workgroup of 16 waves per query, so every row of the pool is gathered from the corpus ONCE.  The K range is
//               cut into chunks of as many k-steps as keep the pool's pieces within 32 KiB of LDS; a chunk's pieces are gathered
//               as they are stored -- a row's 16-byte piece of k-step s, half h is lane (row & 31) + 32 h of the fragment of
//               that k-step, for the A and for the B operand alike, so the staged image of a block of 32 positions IS its A and
//               its B fragment (a wave's ds_read_b128 of one is a contiguous KiB: no bank conflicts).  The next chunk's gather
//               (two pieces per thread) is in flight over the MFMAs of this one.  A wave owns one 32 x 32 tile of G (four when
//               m > 128) and runs ONE chain of v_mfma_f32_32x32x16 on it, k ascending across the chunks from +0.0f: the chain
//               of srx_dense_score_docs_half, with 32 different rows in A where the scorer repeats its query, so no row of a
//               tile is wasted.  Every tile pair (a block, b block) is computed in its own orientation; nothing is mirrored.
//               A dead position's pieces are zeros (no corpus byte is read for it) and its entries are stored as +0.0f.
//   Gram, f32   a kernel of this unit that keeps the order of dense_score.hip: lane l holds columns l, l + 64, ... of a row,
//               products summed in ascending slice order from +0.0f, then the xor butterfly.  A workgroup of 8 waves serves
//               (query, 32 positions a): a wave holds MMR_RA = 4 rows a in registers as "queries"; the pool's rows b pass
//               through LDS MF_BC = 8 at a time (the next eight in flight), so a row is fetched once per workgroup.  The 32
//               lane sums of a round (4 a x 8 b) go through the butterfly TOGETHER: at distance 32 a lane keeps one of two
//               sums and hands the other to its partner, and so on down to distance 2, which halves the registers at every
//               level and costs 32 exchanges for 32 pairs instead of 192.  Each lane still adds, level by level, its own value
//               and the value of lane ^ distance of the same pair: the bits are those of the plain butterfly.
//   select      one wave per query, position c = lane + 64 j in registers (fl(w_rel * rel), pen, open = live and not yet
//               picked, and in cosine mode n[c]).  A step is an arg-max over (v descending, position ascending) by xor
//               shuffles, then COLUMN s of G (S(c, s): candidate first, picked doc second) updates pen.  No LDS.
#include "mmr_common.h"

namespace {

// ================================================================================================ Gram, half
constexpr int MG_THREADS = 1024, MG_WAVES = MG_THREADS / 64;
constexpr int MG_PIECES = 2048;  // pieces of one K chunk in LDS (32 KiB): two per thread
static_assert(MG_PIECES == 2 * MG_THREADS, "a thread of the half Gram kernel moves two pieces per chunk");

template <int TYPE, int TPW>  // TPW: tiles per wave, 1 (at most 16 tiles: m <= 128) or 4
__global__ __launch_bounds__(MG_THREADS) void srx_mmr_gram_half_kernel(MmrArgs a) {
    __shared__ hf_v4i X[MG_PIECES];  // [block of 32 positions][k-step of the chunk][lane]
    __shared__ int rows[SRX_MMR_MAX_M];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int q = (int)blockIdx.x, m = a.m;
    const int nb = (m + 31) >> 5, ks = a.dim >> 4;
    const int kc = MG_PIECES / (nb * 64);  // k-steps per chunk: 32 (one block) .. 4 (eight blocks)
    const hf_v4i *corpus = (const hf_v4i *)a.corpus;
    if (tid < SRX_MMR_MAX_M) rows[tid] = mmr_row(a, q, tid);  // -1 at and past m
    __syncthreads();
    // piece i of a chunk of kcc k-steps that starts at k-step c0: block i / (64 kcc), k-step (i / 64) % kcc, lane i % 64
    hf_v4i pre[2];
    auto gather = [&](int c0, int kcc) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int i = tid + MG_THREADS * j;
            pre[j] = (hf_v4i){0, 0, 0, 0};
            if (i < nb * kcc * 64) {
                const int t = i >> 6, blk = t / kcc, sl = t - blk * kcc;
                const int row = rows[blk * 32 + r];
                if (row >= 0) pre[j] = corpus[hf_piece(row, ks, c0 + sl, h)];
            }
        }
    };
    int ta[TPW], tb[TPW];  // the wave's tiles: (a block, b block), -1 = none
    hf_v16f acc[TPW];
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        const int tile = wave + MG_WAVES * i;
        ta[i] = tile < nb * nb ? tile / nb : -1;
        tb[i] = tile < nb * nb ? tile - ta[i] * nb : -1;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][e] = 0.0f;
    }
    gather(0, min(kc, ks));
    for (int c0 = 0; c0 < ks; c0 += kc) {  // ascending k: one chain per output element
        const int kcc = min(kc, ks - c0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (tid + MG_THREADS * j < nb * kcc * 64) {
                const int i = tid + MG_THREADS * j, t = i >> 6, blk = t / kcc, sl = t - blk * kcc;
                X[(blk * kc + sl) * 64 + lane] = pre[j];
            }
        __syncthreads();
        if (c0 + kc < ks) gather(c0 + kc, min(kc, ks - c0 - kc));  // in flight over this chunk's MFMAs
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            if (ta[i] < 0) continue;  // uniform per wave
            const hf_v4i *A = X + ta[i] * kc * 64 + lane, *B = X + tb[i] * kc * 64 + lane;
            for (int sl = 0; sl < kcc; ++sl) acc[i] = hf_mfma<TYPE>(A[sl * 64], B[sl * 64], acc[i]);
        }
        __syncthreads();  // the chunk has been read: the next one may overwrite it
    }
    // D[row = a][col = b]: lane l holds column l & 31, rows (reg & 3) + 8 (reg >> 2) + 4 (l >> 5)
    float *Gq = a.G + (int64_t)q * m * m;
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
        if (ta[i] < 0) continue;
        const int bpos = tb[i] * 32 + r;
        const bool blive = rows[bpos] >= 0;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int apos = ta[i] * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
            if (apos < m && bpos < m) Gq[(int64_t)apos * m + bpos] = (blive && rows[apos] >= 0) ? acc[i][reg] : 0.0f;
        }
    }
}

// ================================================================================================ Gram, f32
constexpr int MF_THREADS = 512, MF_WAVES = MF_THREADS / 64;
constexpr int MF_AB = MMR_RA * MF_WAVES;  // positions a per workgroup
constexpr int MF_BC = 8;                  // rows b per round
static_assert(MF_AB == 32 && MMR_RA * MF_BC == 32, "the f32 Gram kernel reduces 32 lane sums per round: 4 rows a x 8 rows b");

template <int NS>  // NS: slices of 64 columns held (a bucket >= dim / 64; the slices beyond dim are zeros on both sides and change no bit)
__global__ __launch_bounds__(MF_THREADS) void srx_mmr_gram_f32_kernel(MmrArgs a) {
    constexpr int NJ = NS * 64 * MF_BC / MF_THREADS;  // loads per thread and round (4-byte loads: the rows need no wider alignment)
    constexpr int LD = NS * 64;                       // row stride of the staged rows; columns dim .. LD - 1 are zeros
    __shared__ float Bs[MF_BC * LD];                  // the round's rows b, row-major
    __shared__ int rows[SRX_MMR_MAX_M];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = a.m, dim = a.dim;
    const int nab = (m + MF_AB - 1) / MF_AB;
    const int q = (int)(blockIdx.x / (unsigned)nab), a0 = (int)(blockIdx.x - (unsigned)q * (unsigned)nab) * MF_AB + wave * MMR_RA;
    const float *emb = (const float *)a.corpus;
    if (tid < SRX_MMR_MAX_M) rows[tid] = mmr_row(a, q, tid);  // -1 at and past m
    __syncthreads();
    float qv[MMR_RA][NS];
#pragma unroll
    for (int ai = 0; ai < MMR_RA; ++ai) {
        const int arow = rows[a0 + ai];  // a0 + ai <= 255
        const float *p = emb + (int64_t)(arow >= 0 ? arow : 0) * dim;
#pragma unroll
        for (int i = 0; i < NS; ++i) qv[ai][i] = (arow >= 0 && lane + 64 * i < dim) ? p[lane + 64 * i] : 0.0f;
    }
    float pre[NJ];
    auto fetch = [&](int c0) __attribute__((always_inline)) {  // rows b of positions c0 .. c0 + MF_BC - 1: element f = (row, column)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int f = tid + MF_THREADS * j, bi = f / LD, col = f - bi * LD;  // f < MF_BC * LD
            const int brow = c0 + bi < SRX_MMR_MAX_M ? rows[c0 + bi] : -1;
            pre[j] = 0.0f;
            if (brow >= 0 && col < dim) pre[j] = emb[(int64_t)brow * dim + col];
        }
    };
    float *Gq = a.G + (int64_t)q * m * m;
    fetch(0);
    for (int c0 = 0; c0 < m; c0 += MF_BC) {
#pragma unroll
        for (int j = 0; j < NJ; ++j) Bs[tid + MF_THREADS * j] = pre[j];
        __syncthreads();
        if (c0 + MF_BC < m) fetch(c0 + MF_BC);  // in flight over this round's arithmetic
        float s[MMR_RA * MF_BC];
#pragma unroll
        for (int bi = 0; bi < MF_BC; ++bi) {
            float rv[NS];
#pragma unroll
            for (int i = 0; i < NS; ++i) rv[i] = Bs[bi * LD + lane + 64 * i];
#pragma unroll
            for (int ai = 0; ai < MMR_RA; ++ai) {
                float t = 0.0f;
#pragma unroll
                for (int i = 0; i < NS; ++i) t = t + rv[i] * qv[ai][i];
                s[ai * MF_BC + bi] = t;
            }
        }
        // the butterfly of 32 pairs at once: after the level of distance D, register p holds pair p in the lanes whose bit D is
        // clear and pair p + CNT in the others
#define SRX_MMR_LEVEL(D, CNT)                                                                  \
    _Pragma("unroll") for (int p = 0; p < CNT; ++p) {                                          \
        const bool hi = (lane & D) != 0;                                                       \
        const float keep = hi ? s[p + CNT] : s[p], give = hi ? s[p] : s[p + CNT];              \
        s[p] = keep + __shfl_xor(give, D);                                                     \
    }
        SRX_MMR_LEVEL(32, 16) SRX_MMR_LEVEL(16, 8) SRX_MMR_LEVEL(8, 4) SRX_MMR_LEVEL(4, 2) SRX_MMR_LEVEL(2, 1)
#undef SRX_MMR_LEVEL
        const float g = s[0] + __shfl_xor(s[0], 1);  // lane l: pair l >> 1 = (row a (l >> 4), row b (l >> 1) & 7)
        const int apos = a0 + (lane >> 4), bpos = c0 + ((lane >> 1) & 7);
        if ((lane & 1) == 0 && apos < m && bpos < m) Gq[(int64_t)apos * m + bpos] = (rows[apos] >= 0 && rows[bpos] >= 0) ? g : 0.0f;
        __syncthreads();  // the round has been read: the next one may overwrite it
    }
}

// ================================================================================================ select
constexpr int MMR_NONE = 0x7FFFFFFF;  // "no position" in the arg-max

__global__ __launch_bounds__(THREADS) void srx_mmr_select_kernel(MmrArgs a) {
    const int lane = threadIdx.x & 63;
    const int q = (int)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (q >= a.nq) return;  // whole waves leave
    const int m = a.m, k = a.k;
    const bool cosine = a.sim_mode == SRX_MMR_COSINE;
    const float *Gq = a.G + (int64_t)q * m * m;
    const int32_t *cd = a.cand_doc + (int64_t)q * m;
    const float *cr = a.cand_rel + (int64_t)q * m;
    float wr[MMR_PPL], pen[MMR_PPL], nrm[MMR_PPL];
    bool open[MMR_PPL];  // live and not yet picked
    int n_live = 0;
#pragma unroll
    for (int j = 0; j < MMR_PPL; ++j) {
        const int c = lane + 64 * j;
        open[j] = mmr_row(a, q, c) >= 0;  // false at and past m
        wr[j] = open[j] ? a.w_rel * cr[c] : 0.0f;
        pen[j] = 0.0f;
        nrm[j] = (cosine && open[j]) ? sqrtf(Gq[(int64_t)c * m + c]) : 0.0f;
        n_live += __popcll(__ballot(open[j]));
    }
    const int picks = min(k, n_live);
    int32_t *od = a.out_doc + (int64_t)q * k;
    float *orel = a.out_rel + (int64_t)q * k;
    float *ommr = a.out_mmr != nullptr ? a.out_mmr + (int64_t)q * k : nullptr;
    for (int t = 0; t < picks; ++t) {
        float bv = 0.0f;
        int bc = MMR_NONE;
#pragma unroll
        for (int j = 0; j < MMR_PPL; ++j) {  // ascending position: a strict > keeps the lowest of equal values
            const float v = t == 0 ? wr[j] : wr[j] - a.w_div * pen[j];
            if (open[j] && (bc == MMR_NONE || v > bv)) {
                bv = v;
                bc = lane + 64 * j;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o);
            const int oc = __shfl_xor(bc, o);
            if (oc != MMR_NONE && (bc == MMR_NONE || ov > bv || (ov == bv && oc < bc))) {
                bv = ov;
                bc = oc;
            }
        }
        const int s = __shfl(bc, 0);  // t < picks: an open position exists
        bv = __shfl(bv, 0);
        if (lane == 0) {
            od[t] = cd[s];
            orel[t] = cr[s];
            if (ommr != nullptr) ommr[t] = bv;
        }
        float ns_own = 0.0f;
#pragma unroll
        for (int j = 0; j < MMR_PPL; ++j) {
            if (lane + 64 * j == s) {
                open[j] = false;
                ns_own = nrm[j];
            }
        }
        if (t + 1 == picks) break;
        const float ns = __shfl(ns_own, s & 63);
#pragma unroll
        for (int j = 0; j < MMR_PPL; ++j) {
            if (!open[j]) continue;
            const float g = Gq[(int64_t)(lane + 64 * j) * m + s];  // S(c, s): the candidate first, the picked doc second
            float S = g;
            if (cosine) {
                const float d = nrm[j] * ns;
                S = d > 0.0f ? g / d : 0.0f;
            }
            pen[j] = (t == 0 || S > pen[j]) ? S : pen[j];
        }
    }
    for (int t = picks + lane; t < k; t += 64) {
        od[t] = -1;
        orel[t] = 0.0f;
        if (ommr != nullptr) ommr[t] = 0.0f;
    }
    if (lane == 0) a.out_count[q] = picks;
}

// ================================================================================================ host side
template <int TYPE>
void launch_gram_half(const MmrArgs &a, hipStream_t stream) {
    const dim3 grid((unsigned)a.nq);
    if (a.m <= 128)  // at most 4 x 4 tiles: one per wave
        hipLaunchKernelGGL((srx_mmr_gram_half_kernel<TYPE, 1>), grid, dim3(MG_THREADS), 0, stream, a);
    else
        hipLaunchKernelGGL((srx_mmr_gram_half_kernel<TYPE, 4>), grid, dim3(MG_THREADS), 0, stream, a);
}

void launch_gram_f32(const MmrArgs &a, hipStream_t stream) {
    const int ns = a.dim / 64;
    const dim3 grid((unsigned)((int64_t)a.nq * ((a.m + MF_AB - 1) / MF_AB)));  // <= nq * m < 2^31
#define SRX_MF(NS)                                                                                                     \
    if (ns <= NS) {                                                                                                    \
        hipLaunchKernelGGL((srx_mmr_gram_f32_kernel<NS>), grid, dim3(MF_THREADS), 0, stream, a);                       \
        return;                                                                                                        \
    }
    SRX_MF(1) SRX_MF(2) SRX_MF(4) SRX_MF(8) SRX_MF(12) SRX_MF(16)
#undef SRX_MF
}

bool weight_ok(float w) { return w >= 0.0f && w <= 3.402823466e+38f; }  // false for a NaN, an infinity, a negative value

// type < 0: the f32 form
int mmr_select(const char *who, int32_t type, int32_t device, const void *corpus, int64_t n_docs, int32_t dim, int64_t doc_base,
               const int32_t *cand_doc, const float *cand_rel, const int32_t *cand_count, int32_t nq, int32_t m, int32_t k, int32_t sim_mode,
               float w_rel, float w_div, int32_t *out_doc, float *out_rel, float *out_mmr, int32_t *out_count, float *out_sim, void *workspace,
               int64_t workspace_bytes, void *stream_v) {
    if (m < 1 || m > SRX_MMR_MAX_M) return fail(SRX_ERR_INVALID, "%s: m must be in 1 .. 256", who);
    if (k < 1 || k > m) return fail(SRX_ERR_INVALID, "%s: k must be in 1 .. m", who);
    if (sim_mode != SRX_MMR_DOT && sim_mode != SRX_MMR_COSINE) return fail(SRX_ERR_INVALID, "%s: sim_mode must be SRX_MMR_DOT or SRX_MMR_COSINE", who);
    if (!weight_ok(w_rel) || !weight_ok(w_div)) return fail(SRX_ERR_INVALID, "%s: the weights must be finite and >= 0", who);
    if (w_rel == 0.0f && w_div == 0.0f) return fail(SRX_ERR_INVALID, "%s: the weights are both 0", who);
    if (!hf_dim_ok(dim)) return fail(SRX_ERR_INVALID, "%s: the row length must be a multiple of 64, <= 1024 (pad the rows with zeros)", who);
    if (n_docs <= 0 || n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: n_docs out of range", who);
    if (doc_base < 0) return fail(SRX_ERR_INVALID, "%s: doc_base < 0", who);
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if ((int64_t)nq * (int64_t)m > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: nq * m must fit int32", who);
    if (nq == 0) return SRX_OK;
    if (!corpus || !cand_doc || !cand_rel || !out_doc || !out_rel || !out_count) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (type >= 0 && ((uintptr_t)corpus & 15)) return fail(SRX_ERR_INVALID, "%s: the corpus must be 16-byte aligned", who);
    // G goes to out_sim when that is given (the workspace may then be that very buffer: no alignment slack is needed)
    const int64_t need = mmr_gram_bytes(nq, m) + (out_sim != nullptr ? 0 : 256);
    if (!workspace || workspace_bytes < need) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    HIP_TRY(hipSetDevice(device));
    float *G = out_sim != nullptr ? out_sim : (float *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    const MmrArgs a = {corpus, cand_doc, cand_rel, cand_count, G, out_doc, out_rel, out_mmr, out_count, n_docs, doc_base, nq, m, k, dim, sim_mode, w_rel, w_div};
    hipStream_t stream = (hipStream_t)stream_v;
    if (type == SRX_HALF_F16)
        launch_gram_half<SRX_HALF_F16>(a, stream);
    else if (type == SRX_HALF_BF16)
        launch_gram_half<SRX_HALF_BF16>(a, stream);
    else
        launch_gram_f32(a, stream);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(srx_mmr_select_kernel, dim3((unsigned)((nq + WAVES - 1) / WAVES)), dim3(THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

}  // namespace

SRX_API int64_t srx_mmr_workspace_bytes(int32_t nq, int32_t m) {
    if (nq < 0 || m < 1 || m > SRX_MMR_MAX_M) return fail(SRX_ERR_INVALID, "srx_mmr_workspace_bytes: need nq >= 0 and m in 1 .. 256%s");
    return mmr_gram_bytes(nq, m) + 256;
}

SRX_API int srx_mmr_select_f32(int32_t device, const float *emb, int64_t n_docs, int32_t dim, int64_t doc_base, const int32_t *cand_doc,
                               const float *cand_rel, const int32_t *cand_count, int32_t nq, int32_t m, int32_t k, int32_t sim_mode, float w_rel,
                               float w_div, int32_t *out_doc, float *out_rel, float *out_mmr, int32_t *out_count, float *out_sim, void *workspace,
                               int64_t workspace_bytes, void *stream) {
    return mmr_select("srx_mmr_select_f32", -1, device, emb, n_docs, dim, doc_base, cand_doc, cand_rel, cand_count, nq, m, k, sim_mode, w_rel, w_div,
                      out_doc, out_rel, out_mmr, out_count, out_sim, workspace, workspace_bytes, stream);
}

SRX_API int srx_mmr_select_half(int32_t device, int32_t type, const void *corpus_packed, int64_t n_docs, int32_t dim_pad, int64_t doc_base,
                                const int32_t *cand_doc, const float *cand_rel, const int32_t *cand_count, int32_t nq, int32_t m, int32_t k,
                                int32_t sim_mode, float w_rel, float w_div, int32_t *out_doc, float *out_rel, float *out_mmr, int32_t *out_count,
                                float *out_sim, void *workspace, int64_t workspace_bytes, void *stream) {
    const char *who = "srx_mmr_select_half";
    if (type != SRX_HALF_F16 && type != SRX_HALF_BF16) return fail(SRX_ERR_INVALID, "%s: type must be SRX_HALF_F16 or SRX_HALF_BF16", who);
    return mmr_select(who, type, device, corpus_packed, n_docs, dim_pad, doc_base, cand_doc, cand_rel, cand_count, nq, m, k, sim_mode, w_rel, w_div,
                      out_doc, out_rel, out_mmr, out_count, out_sim, workspace, workspace_bytes, stream);
}
