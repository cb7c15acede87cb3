// fuse.hip -- hybrid retrieval: fuse a sparse and a dense ranked top-k list per query into one ranked list
// (srx_fuse_topk).  Same build flags as the other units; -ffp-contract=off matters here too: a contribution is one
// IEEE divide and one multiply (weighted) or one add and one divide (rrf), and the fused score one add.
//
//   wave form   ka + kb <= FW_CAP (1024) and k <= W_KMAX (128): one wavefront per query, no block barrier.  The used
//               entries of list A are compacted into the wave's LDS list and their list positions entered into an
//               open-addressing table keyed by doc id; list B probes it: a hit adds its contribution to A's entry, a
//               miss is appended.  wave_list_select / wave_rank_emit (srx_common.h) select, rank and write the row.
//               A NaN contribution never enters the list (the selection orders by unsigned bits, and NaN bits sort above
//               +inf): A's entry is parked instead -- doc only, at the far end of the list, entered into the table -- so
//               that B's copy is found and dropped; B's NaN is dropped on a miss, and on a hit the sum turns A's entry
//               NaN and one compaction pass (fuse_wave_drop_nan, only then) takes such entries out.
//   block form  everything else (<= 2048 candidates, k <= 1024): one 256-thread workgroup per query, candidates in
//               registers, the same table (aliasing the selection histogram, which is only needed afterwards), topk_fold
//               keeps the k best and block_rank_emit ranks and writes the row (both srx_common.h: the selection and
//               ranking of the merge kernel, not a second copy).  A's entries with a NaN contribution are entered like the
//               others, B's probe like the others; the sum of an entry is formed in registers, and a NaN there is no
//               candidate.
// A contribution is NaN only in mode weighted: +inf / +inf, or a zero weight times an infinite quotient.  The contract's
// c_A + c_B is then NaN, not > 0: the doc is in no result, whichever list the NaN comes from -- as in the scored form below.
// The table holds positions, not keys (the key of slot value v is the doc stored at position v - 1), so a slot is one
// word: 8 KiB for 2048 slots, load <= 0.5 because only list A (< 1024 / <= 1024 entries) is entered.
#include "srx_common.h"

namespace {

constexpr int FW_CAP = 1024;                // wave form: candidate slots (= MW_CAP of the merge wave kernel)
constexpr int FW_NPL = FW_CAP / 64;         // per lane
constexpr int FB_CAP = 2 * KMAX;            // block form: candidate slots
constexpr int FB_NPT = FB_CAP / THREADS;    // per thread (8)
constexpr int F_SLOTS = 2048;               // table slots (a power of two, > 2 * entries of list A in the wave form,
                                            // >= 2 * entries in the block form)
constexpr int F_SLOT_BITS = 11;
static_assert(F_SLOTS == (1 << F_SLOT_BITS) && F_SLOTS >= 2 * KMAX && F_SLOTS <= RADIX_BINS, "table size");

struct FuseArgs {
    const int32_t *a_doc, *b_doc;
    const float *a_score, *b_score;
    const int32_t *a_count, *b_count;
    int32_t *out_doc;
    float *out_score;
    int32_t *out_count;
    int nq, ka, kb, k, mode;
    float wa, wb, rrf_c;
};

__device__ __forceinline__ unsigned fuse_slot(int doc) { return ((unsigned)doc * 2654435761u) >> (32 - F_SLOT_BITS); }

// contribution of entry r (score s) of a list with weight w and best score m; 0 = not used
__device__ __forceinline__ float fuse_contribution(int mode, bool used, float w, float s, float m, int r, float rrf_c) {
    if (!used) return 0.0f;
    if (mode == SRX_FUSE_WEIGHTED) return w * (s / m);
    return w / (rrf_c + (float)(r + 1));
}

// Enter position p (0-based; its doc is already stored where `doc_at` finds it) under `doc`.  Terminates: at most
// F_SLOTS / 2 entries are ever entered, so an empty slot exists.
__device__ __forceinline__ void fuse_insert(unsigned *tbl, int doc, unsigned p) {
    unsigned h = fuse_slot(doc);
    while (atomicCAS(&tbl[h], 0u, p + 1u) != 0u) h = (h + 1u) & (F_SLOTS - 1);
}
// position of `doc` among the entered entries, or -1
template <typename DocAt>
__device__ __forceinline__ int fuse_find(const unsigned *tbl, int doc, DocAt doc_at) {
    unsigned h = fuse_slot(doc);
    for (int n = 0; n < F_SLOTS; ++n) {  // bounded even if the table were full
        const unsigned v = tbl[h];
        if (v == 0u) return -1;
        if (doc_at(v - 1u) == doc) return (int)(v - 1u);
        h = (h + 1u) & (F_SLOTS - 1);
    }
    return -1;
}

// the head of a list decides whether mode `weighted` uses the list at all, and is its divisor
__device__ __forceinline__ float fuse_head(const int32_t *doc, const float *score, int cnt, int64_t row0) {
    if (cnt <= 0) return 0.0f;
    const float m = score[row0];
    return (doc[row0] >= 0 && m > 0.0f) ? m : 0.0f;
}

struct FuseWaveShared {
    static constexpr bool HIST_ALIASES_ZEROED_LDS = false;
    unsigned lbits[FW_CAP];
    int ldoc[FW_CAP];
    unsigned hist[256];
    unsigned long long sortkey[128];
    unsigned tbl[F_SLOTS];
};  // 18 KiB per wave, 72 KiB per workgroup: two workgroups per CU

// Take the NaN entries out of the wave's list (count entries in S.lbits / S.ldoc), in place; returns the new count.  Rare, so
// not inlined.  The compaction of wave_list_select: 64 entries per step are read before any is written, and an entry only
// moves down.
__device__ __noinline__ unsigned fuse_wave_drop_nan(FuseWaveShared &S, unsigned count) {
    const int lane = threadIdx.x & 63;
    unsigned base = 0;  // wave-uniform running count
    for (unsigned i0 = 0; i0 < count; i0 += 64) {
        const unsigned i = i0 + lane;
        const unsigned x = i < count ? S.lbits[i] : 0u;
        const int dd = i < count ? S.ldoc[i] : 0;
        const bool take = i < count && (x & 0x7FFFFFFFu) <= 0x7F800000u;
        const unsigned long long m = __ballot(take);
        wsync();
        if (take) {
            const unsigned p = base + lane_rank(m);
            S.lbits[p] = x;
            S.ldoc[p] = dd;
        }
        base += (unsigned)__popcll(m);
        wsync();
    }
    return base;
}

__global__ __launch_bounds__(THREADS) void srx_fuse_wave_kernel(FuseArgs a) {
    __shared__ FuseWaveShared FW[WAVES];
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (q >= a.nq) return;  // whole waves leave; nothing below is a block barrier
    FuseWaveShared &S = FW[threadIdx.x >> 6];
    const int ka = a.ka, kb = a.kb, k = a.k;
    const int64_t a0 = (int64_t)q * ka, b0 = (int64_t)q * kb;
    // round trip 1: the counts; round trip 2: the heads and every used slot of both rows
    const int ca = max(0, min(a.a_count[q], ka)), cb = max(0, min(a.b_count[q], kb));
    float ma = 1.0f, mb = 1.0f;
    bool a_on = true, b_on = true;
    if (a.mode == SRX_FUSE_WEIGHTED) {
        ma = fuse_head(a.a_doc, a.a_score, ca, a0);
        mb = fuse_head(a.b_doc, a.b_score, cb, b0);
        a_on = ma > 0.0f;
        b_on = mb > 0.0f;
    }
    float sc[FW_NPL];
    int dd[FW_NPL];
#pragma unroll
    for (int j = 0; j < FW_NPL; ++j) {
        const int c = j * 64 + lane;
        sc[j] = 0.0f;
        dd[j] = -1;
        if (c < ka) {
            if (c < ca) {
                sc[j] = a.a_score[a0 + c];
                dd[j] = a.a_doc[a0 + c];
            }
        } else if (c - ka < cb) {
            sc[j] = a.b_score[b0 + (c - ka)];
            dd[j] = a.b_doc[b0 + (c - ka)];
        }
    }
#pragma unroll
    for (int j = 0; j < F_SLOTS / 256; ++j) reinterpret_cast<uint4 *>(S.tbl)[j * 64 + lane] = make_uint4(0u, 0u, 0u, 0u);
    wsync();
    // contributions: +0 = drop (unused entry, zero weight or underflow; adding it would not change the other side's bits),
    // NaN (weighted only: +inf / +inf, or a zero weight times an infinite quotient) = the doc leaves the result
    bool a_nan = false;
#pragma unroll
    for (int j = 0; j < FW_NPL; ++j) {
        const int c = j * 64 + lane;
        const bool is_a = c < ka;
        const bool used = dd[j] >= 0 && sc[j] > 0.0f && (is_a ? a_on : b_on);
        sc[j] = fuse_contribution(a.mode, used, is_a ? a.wa : a.wb, sc[j], is_a ? ma : mb, is_a ? c : c - ka, a.rrf_c);
        a_nan |= is_a && sc[j] != sc[j];
    }
    // list A: compact into the list, enter the positions
    unsigned count = 0;  // wave-uniform
#pragma unroll
    for (int j = 0; j < FW_NPL; ++j) {
        if (j * 64 >= ka) break;
        const bool ok = j * 64 + lane < ka && sc[j] > 0.0f;
        const unsigned long long m = __ballot(ok);
        if (ok) {
            const unsigned p = count + lane_rank(m);
            S.lbits[p] = __float_as_uint(sc[j]);
            S.ldoc[p] = dd[j];
            fuse_insert(S.tbl, dd[j], p);  // claims a slot only: keys are compared by the probes, after the wsync below
        }
        count += (unsigned)__popcll(m);
    }
    const unsigned na = count;
    // A's entries with a NaN contribution are parked, docs only, from the list's last slot downwards and entered too, so that
    // B's copy of such a doc is found and dropped.  They never meet the list: entries of A + parked <= ka, appended <= kb.
    unsigned parked = 0;  // wave-uniform
    if (__ballot(a_nan) != 0ull) {
#pragma unroll
        for (int j = 0; j < FW_NPL; ++j) {
            if (j * 64 >= ka) break;
            const bool ok = j * 64 + lane < ka && sc[j] != sc[j];
            const unsigned long long m = __ballot(ok);
            if (ok) {
                const unsigned p = (unsigned)(FW_CAP - 1) - (parked + lane_rank(m));
                S.ldoc[p] = dd[j];
                fuse_insert(S.tbl, dd[j], p);
            }
            parked += (unsigned)__popcll(m);
        }
    }
    wsync();
    // list B: a hit adds to A's entry (docs are unique inside B, so no two lanes hit the same entry) unless that entry is
    // parked, a miss is appended unless it is NaN.  A NaN that hits makes A's entry NaN: such entries are taken out below.
    bool nan_hit = false;
#pragma unroll
    for (int j = 0; j < FW_NPL; ++j) {
        if ((j + 1) * 64 <= ka) continue;
        const bool isb = j * 64 + lane >= ka && sc[j] != 0.0f;  // > 0 or NaN
        const bool b_nan = sc[j] != sc[j];
        int hit = -1;
        if (isb && na + parked > 0) hit = fuse_find(S.tbl, dd[j], [&](unsigned p) -> int { return S.ldoc[p]; });
        const bool add = isb && hit >= 0 && hit < (int)na;
        if (add) S.lbits[hit] = __float_as_uint(__uint_as_float(S.lbits[hit]) + sc[j]);
        nan_hit |= add && b_nan;
        const bool app = isb && hit < 0 && !b_nan;
        const unsigned long long m = __ballot(app);
        if (app) {
            const unsigned p = count + lane_rank(m);
            S.lbits[p] = __float_as_uint(sc[j]);
            S.ldoc[p] = dd[j];
        }
        count += (unsigned)__popcll(m);
    }
    wsync();
    if (__ballot(nan_hit) != 0ull) count = fuse_wave_drop_nan(S, count);
    if (count > (unsigned)k) {
        wave_list_select(S, count, k);
        count = (unsigned)k;
    }
    wave_rank_emit(S, S.sortkey, count, k, (int64_t)0, a.out_doc + (int64_t)q * k, a.out_score + (int64_t)q * k);
    if (lane == 0) a.out_count[q] = (int)count;
}

struct FuseBlockShared {
    TopkShared tk;
    unsigned hist[RADIX_BINS];           // first the table, then topk_fold's histogram
    unsigned long long sortkey[KMAX];    // first list A by rank -- adoc[KMAX]: doc (the table's keys), addc[KMAX]: what list B
                                         // adds to it -- then block_rank_emit's sort keys
};  // ~24.1 KiB per workgroup

__global__ __launch_bounds__(THREADS) void srx_fuse_block_kernel(FuseArgs a) {
    __shared__ FuseBlockShared S;
    int *const adoc = reinterpret_cast<int *>(S.sortkey);
    float *const addc = reinterpret_cast<float *>(S.sortkey) + KMAX;
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    const int ka = a.ka, kb = a.kb, k = a.k;
    const int64_t a0 = (int64_t)q * ka, b0 = (int64_t)q * kb;
    const int ca = max(0, min(a.a_count[q], ka)), cb = max(0, min(a.b_count[q], kb));
    float ma = 1.0f, mb = 1.0f;
    bool a_on = true, b_on = true;
    if (a.mode == SRX_FUSE_WEIGHTED) {
        ma = fuse_head(a.a_doc, a.a_score, ca, a0);
        mb = fuse_head(a.b_doc, a.b_score, cb, b0);
        a_on = ma > 0.0f;
        b_on = mb > 0.0f;
    }
    float sc[FB_NPT];
    int dd[FB_NPT];
#pragma unroll
    for (int n = 0; n < FB_NPT; ++n) {
        const int c = n * THREADS + tid;
        sc[n] = 0.0f;
        dd[n] = -1;
        if (c < ka) {
            if (c < ca) {
                sc[n] = a.a_score[a0 + c];
                dd[n] = a.a_doc[a0 + c];
            }
        } else if (c - ka < cb) {
            sc[n] = a.b_score[b0 + (c - ka)];
            dd[n] = a.b_doc[b0 + (c - ka)];
        }
    }
    for (int i = tid; i < F_SLOTS; i += THREADS) S.hist[i] = 0u;
    for (int i = tid; i < KMAX; i += THREADS) addc[i] = 0.0f;
    if (tid == 0) {
        S.tk.count = 0;
        S.tk.tau = 0;
    }
#pragma unroll
    for (int n = 0; n < FB_NPT; ++n) {
        const int c = n * THREADS + tid;
        const bool is_a = c < ka;
        const bool used = dd[n] >= 0 && sc[n] > 0.0f && (is_a ? a_on : b_on);
        sc[n] = fuse_contribution(a.mode, used, is_a ? a.wa : a.wb, sc[n], is_a ? ma : mb, is_a ? c : c - ka, a.rrf_c);
        if (is_a && sc[n] != 0.0f) adoc[c] = dd[n];  // > 0 or NaN (see the wave form); c = rank in A < ka <= KMAX
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < FB_NPT; ++n) {
        const int c = n * THREADS + tid;
        if (c < ka && sc[n] != 0.0f) fuse_insert(S.hist, dd[n], (unsigned)c);
    }
    __syncthreads();
    unsigned ubits[FB_NPT];
    int udoc[FB_NPT];
#pragma unroll
    for (int n = 0; n < FB_NPT; ++n) {
        const int c = n * THREADS + tid;
        if (c >= ka && sc[n] != 0.0f) {
            const int hit = fuse_find(S.hist, dd[n], [&](unsigned p) -> int { return adoc[p]; });
            if (hit >= 0) {
                addc[hit] = sc[n];  // docs are unique inside B: one writer per entry of A; a NaN makes A's entry NaN
                sc[n] = 0.0f;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < FB_NPT; ++n) {
        const int c = n * THREADS + tid;
        float f = sc[n];
        if (c < ka && f > 0.0f) f = f + addc[c];
        ubits[n] = f > 0.0f ? __float_as_uint(f) : 0u;  // a NaN, from either list, is no candidate
        udoc[n] = dd[n];
    }
    __syncthreads();  // the table and list A's arrays are dead: their words become the selection histogram and the sort keys
    topk_fold<FB_NPT, false>(ubits, udoc, k, S.tk, S.hist);
    block_rank_emit(S.tk, S.sortkey, k, (int64_t)0, a.out_doc + (int64_t)q * k, a.out_score + (int64_t)q * k, a.out_count + q);
}

// ---- fusion of two COMPLETED lists (srx_fuse_topk_scored, include/sparse_rx_rescore.h) -----------------------------------
// Every entry carries the other side's score of its doc (`*_other`), so no contribution crosses between the lists: the
// table only finds the entries of list B whose doc list A holds as well, and those are dropped.  The same two forms, the
// same table, selection and ranking as above.
struct FuseScoredArgs {
    FuseArgs f;  // mode = SRX_FUSE_WEIGHTED
    const float *a_other, *b_other;
};
// The heads of the two lists and what an entry fuses to
struct FuseScoredSides {
    float wa, wb, ma, mb;  // m = 0: the side has no normaliser and contributes nothing anywhere
    // a score on side A / B: its contribution, or +0 (adding +0 changes no bit of a value >= 0)
    __device__ __forceinline__ float from_a(float s) const { return (ma > 0.0f && s > 0.0f) ? wa * (s / ma) : 0.0f; }
    __device__ __forceinline__ float from_b(float s) const { return (mb > 0.0f && s > 0.0f) ? wb * (s / mb) : 0.0f; }
};
// Candidate c of query q (c < ka: list A's entry c, else list B's entry c - ka): its doc, or -1 when the entry is not used,
// and its fused score (two operands: the order of the sum does not matter)
__device__ __forceinline__ void fuse_scored_load(const FuseScoredArgs &s, const FuseScoredSides &w, int c, int ca, int cb, int64_t a0,
                                                 int64_t b0, int &doc, float &fused) {
    const FuseArgs &a = s.f;
    float sa = 0.0f, sb = 0.0f, own = 0.0f;
    doc = -1;
    if (c < a.ka) {
        if (c < ca) {
            own = sa = a.a_score[a0 + c];
            sb = s.a_other[a0 + c];
            doc = a.a_doc[a0 + c];
        }
    } else if (c - a.ka < cb) {
        own = sb = a.b_score[b0 + (c - a.ka)];
        sa = s.b_other[b0 + (c - a.ka)];
        doc = a.b_doc[b0 + (c - a.ka)];
    }
    if (!(own > 0.0f)) doc = -1;
    fused = doc >= 0 ? w.from_a(sa) + w.from_b(sb) : 0.0f;
}

__global__ __launch_bounds__(THREADS) void srx_fuse_scored_wave_kernel(FuseScoredArgs s) {
    __shared__ FuseWaveShared FW[WAVES];
    const FuseArgs &a = s.f;
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (q >= a.nq) return;  // whole waves leave; nothing below is a block barrier
    FuseWaveShared &S = FW[threadIdx.x >> 6];
    const int ka = a.ka, kb = a.kb, k = a.k;
    const int64_t a0 = (int64_t)q * ka, b0 = (int64_t)q * kb;
    const int ca = max(0, min(a.a_count[q], ka)), cb = max(0, min(a.b_count[q], kb));
    const FuseScoredSides w = {a.wa, a.wb, fuse_head(a.a_doc, a.a_score, ca, a0), fuse_head(a.b_doc, a.b_score, cb, b0)};
    float sc[FW_NPL];  // fused score
    int dd[FW_NPL];    // doc; -1 = entry not used
#pragma unroll
    for (int j = 0; j < FW_NPL; ++j) fuse_scored_load(s, w, j * 64 + lane, ca, cb, a0, b0, dd[j], sc[j]);
#pragma unroll
    for (int j = 0; j < F_SLOTS / 256; ++j) reinterpret_cast<uint4 *>(S.tbl)[j * 64 + lane] = make_uint4(0u, 0u, 0u, 0u);
    wsync();
    // list A: the entries that rank (fused score > 0) are compacted into the list and entered; the used entries that do
    // not rank are parked behind them, docs only, and entered too: a duplicate in B is dropped whatever A's entry fuses to
    unsigned count = 0;  // wave-uniform
#pragma unroll
    for (int j = 0; j < FW_NPL; ++j) {
        if (j * 64 >= ka) break;
        const bool ok = j * 64 + lane < ka && sc[j] > 0.0f;
        const unsigned long long m = __ballot(ok);
        if (ok) {
            const unsigned p = count + lane_rank(m);
            S.lbits[p] = __float_as_uint(sc[j]);
            S.ldoc[p] = dd[j];
            fuse_insert(S.tbl, dd[j], p);  // claims a slot only: keys are compared by the probes, after the wsync below
        }
        count += (unsigned)__popcll(m);
    }
    unsigned parked = count;
#pragma unroll
    for (int j = 0; j < FW_NPL; ++j) {
        if (j * 64 >= ka) break;
        const bool ok = j * 64 + lane < ka && dd[j] >= 0 && !(sc[j] > 0.0f);
        const unsigned long long m = __ballot(ok);
        if (ok) {
            const unsigned p = parked + lane_rank(m);
            S.ldoc[p] = dd[j];
            fuse_insert(S.tbl, dd[j], p);
        }
        parked += (unsigned)__popcll(m);
    }
    wsync();
    // list B: every probe first (the parked docs are still in place), then the misses are appended over the parked docs
#pragma unroll
    for (int j = 0; j < FW_NPL; ++j) {
        if ((j + 1) * 64 <= ka) continue;
        const bool isb = j * 64 + lane >= ka && sc[j] > 0.0f;
        if (isb && parked > 0 && fuse_find(S.tbl, dd[j], [&](unsigned p) -> int { return S.ldoc[p]; }) >= 0) sc[j] = 0.0f;
    }
    wsync();
#pragma unroll
    for (int j = 0; j < FW_NPL; ++j) {
        if ((j + 1) * 64 <= ka) continue;
        const bool app = j * 64 + lane >= ka && sc[j] > 0.0f;
        const unsigned long long m = __ballot(app);
        if (app) {
            const unsigned p = count + lane_rank(m);
            S.lbits[p] = __float_as_uint(sc[j]);
            S.ldoc[p] = dd[j];
        }
        count += (unsigned)__popcll(m);
    }
    wsync();
    if (count > (unsigned)k) {
        wave_list_select(S, count, k);
        count = (unsigned)k;
    }
    wave_rank_emit(S, S.sortkey, count, k, (int64_t)0, a.out_doc + (int64_t)q * k, a.out_score + (int64_t)q * k);
    if (lane == 0) a.out_count[q] = (int)count;
}

__global__ __launch_bounds__(THREADS) void srx_fuse_scored_block_kernel(FuseScoredArgs s) {
    __shared__ FuseBlockShared S;
    const FuseArgs &a = s.f;
    int *const adoc = reinterpret_cast<int *>(S.sortkey);  // list A by rank: the table's keys
    const int tid = threadIdx.x;
    const int q = blockIdx.x;
    const int ka = a.ka, kb = a.kb, k = a.k;
    const int64_t a0 = (int64_t)q * ka, b0 = (int64_t)q * kb;
    const int ca = max(0, min(a.a_count[q], ka)), cb = max(0, min(a.b_count[q], kb));
    const FuseScoredSides w = {a.wa, a.wb, fuse_head(a.a_doc, a.a_score, ca, a0), fuse_head(a.b_doc, a.b_score, cb, b0)};
    float sc[FB_NPT];
    int dd[FB_NPT];
#pragma unroll
    for (int n = 0; n < FB_NPT; ++n) fuse_scored_load(s, w, n * THREADS + tid, ca, cb, a0, b0, dd[n], sc[n]);
    for (int i = tid; i < F_SLOTS; i += THREADS) S.hist[i] = 0u;
    if (tid == 0) {
        S.tk.count = 0;
        S.tk.tau = 0;
    }
#pragma unroll
    for (int n = 0; n < FB_NPT; ++n) {
        const int c = n * THREADS + tid;
        if (c < ka && dd[n] >= 0) adoc[c] = dd[n];  // every used entry of A, whatever it fuses to
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < FB_NPT; ++n) {
        const int c = n * THREADS + tid;
        if (c < ka && dd[n] >= 0) fuse_insert(S.hist, dd[n], (unsigned)c);
    }
    __syncthreads();
    unsigned ubits[FB_NPT];
    int udoc[FB_NPT];
#pragma unroll
    for (int n = 0; n < FB_NPT; ++n) {
        const int c = n * THREADS + tid;
        if (c >= ka && sc[n] > 0.0f && fuse_find(S.hist, dd[n], [&](unsigned p) -> int { return adoc[p]; }) >= 0) sc[n] = 0.0f;
        ubits[n] = sc[n] > 0.0f ? __float_as_uint(sc[n]) : 0u;
        udoc[n] = dd[n];
    }
    __syncthreads();  // the table and list A's docs are dead: their words become the selection histogram and the sort keys
    topk_fold<FB_NPT, false>(ubits, udoc, k, S.tk, S.hist);
    block_rank_emit(S.tk, S.sortkey, k, (int64_t)0, a.out_doc + (int64_t)q * k, a.out_score + (int64_t)q * k, a.out_count + q);
}

}  // namespace

SRX_API int srx_fuse_topk(int32_t device, const int32_t *a_doc, const float *a_score, const int32_t *a_count, int32_t ka,
                          const int32_t *b_doc, const float *b_score, const int32_t *b_count, int32_t kb, int32_t nq,
                          int32_t k, int32_t mode, float weight_a, float weight_b, float rrf_c, int32_t *out_doc,
                          float *out_score, int32_t *out_count, void *stream_v) {
    if (nq < 0) return fail(SRX_ERR_INVALID, "srx_fuse_topk: nq < 0%s");
    if (ka < 1 || ka > KMAX || kb < 1 || kb > KMAX) return fail(SRX_ERR_INVALID, "srx_fuse_topk: ka / kb must be in 1..1024%s");
    if (k < 1 || k > KMAX) return fail(SRX_ERR_INVALID, "srx_fuse_topk: k must be in 1..1024%s");
    if (mode != SRX_FUSE_WEIGHTED && mode != SRX_FUSE_RRF) return fail(SRX_ERR_INVALID, "srx_fuse_topk: unknown mode%s");
    if (!isfinite(weight_a) || !isfinite(weight_b) || weight_a < 0.0f || weight_b < 0.0f)
        return fail(SRX_ERR_INVALID, "srx_fuse_topk: weights must be finite and >= 0%s");
    if (weight_a == 0.0f && weight_b == 0.0f) return fail(SRX_ERR_INVALID, "srx_fuse_topk: both weights are 0%s");
    if (mode == SRX_FUSE_RRF && !(isfinite(rrf_c) && rrf_c > 0.0f))
        return fail(SRX_ERR_INVALID, "srx_fuse_topk: rrf_c must be finite and > 0%s");
    if (nq == 0) return SRX_OK;
    if (!a_doc || !a_score || !a_count || !b_doc || !b_score || !b_count || !out_doc || !out_score || !out_count)
        return fail(SRX_ERR_INVALID, "srx_fuse_topk: null pointer%s");
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    const FuseArgs a = {a_doc, b_doc, a_score, b_score, a_count, b_count, out_doc, out_score, out_count,
                        nq, ka, kb, k, mode, weight_a, weight_b, rrf_c};
    if (ka + kb <= FW_CAP && k <= W_KMAX) {
        hipLaunchKernelGGL(srx_fuse_wave_kernel, dim3((unsigned)((nq + WAVES - 1) / WAVES)), dim3(THREADS), 0, stream, a);
        HIP_TRY(hipGetLastError());
        return SRX_OK;
    }
    hipLaunchKernelGGL(srx_fuse_block_kernel, dim3((unsigned)nq), dim3(THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

#include "sparse_rx_rescore.h"

SRX_API int srx_fuse_topk_scored(int32_t device, const int32_t *a_doc, const float *a_score, const float *a_other,
                                 const int32_t *a_count, int32_t ka, const int32_t *b_doc, const float *b_score,
                                 const float *b_other, const int32_t *b_count, int32_t kb, int32_t nq, int32_t k, float weight_a,
                                 float weight_b, int32_t *out_doc, float *out_score, int32_t *out_count, void *stream_v) {
    if (nq < 0) return fail(SRX_ERR_INVALID, "srx_fuse_topk_scored: nq < 0%s");
    if (ka < 1 || ka > KMAX || kb < 1 || kb > KMAX) return fail(SRX_ERR_INVALID, "srx_fuse_topk_scored: ka / kb must be in 1..1024%s");
    if (k < 1 || k > KMAX) return fail(SRX_ERR_INVALID, "srx_fuse_topk_scored: k must be in 1..1024%s");
    if (!isfinite(weight_a) || !isfinite(weight_b) || weight_a < 0.0f || weight_b < 0.0f)
        return fail(SRX_ERR_INVALID, "srx_fuse_topk_scored: weights must be finite and >= 0%s");
    if (weight_a == 0.0f && weight_b == 0.0f) return fail(SRX_ERR_INVALID, "srx_fuse_topk_scored: both weights are 0%s");
    if (nq == 0) return SRX_OK;
    if (!a_doc || !a_score || !a_other || !a_count || !b_doc || !b_score || !b_other || !b_count || !out_doc || !out_score || !out_count)
        return fail(SRX_ERR_INVALID, "srx_fuse_topk_scored: null pointer%s");
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    const FuseScoredArgs s = {{a_doc, b_doc, a_score, b_score, a_count, b_count, out_doc, out_score, out_count, nq, ka, kb, k,
                               SRX_FUSE_WEIGHTED, weight_a, weight_b, 0.0f},
                              a_other, b_other};
    if (ka + kb <= FW_CAP && k <= W_KMAX)  // the dispatch rule of srx_fuse_topk
        hipLaunchKernelGGL(srx_fuse_scored_wave_kernel, dim3((unsigned)((nq + WAVES - 1) / WAVES)), dim3(THREADS), 0, stream, s);
    else
        hipLaunchKernelGGL(srx_fuse_scored_block_kernel, dim3((unsigned)nq), dim3(THREADS), 0, stream, s);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
