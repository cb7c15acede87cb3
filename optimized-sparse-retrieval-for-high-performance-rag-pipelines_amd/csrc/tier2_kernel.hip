// tier2_kernel.hip -- tier 2 of the sparse search: a persistent grid of 256-thread workgroups drains the worklist of
// (query, split) blocks tier 1 (wave_kernel.hip) could not finish: flagged units (long runs, many multi-term docs), queries
// of > 64 terms, k > 112, unit overrides, search-after.  Handles everything.
//
// Replaces simd_bm25_score + fast_topk_selection (rag_system/core/retrieval.py:41-92) / simd_tfidf_score
// (rag_system/pipeline/evaluate_rag_pipeline.py:95-121) where tier 1 does not.
//
// Per block: block-level LDS hash units of up to 4096 postings, a greedy tile packer, and dense fp32 accumulators acc[G]
// in LDS for tiles whose postings exceed that (a barrier between terms keeps the summation order).  No MFMA (sparse
// gather/reduce, HBM-bound), no float atomics (LDS ds_add_f32 serialises at ~192 cycles per wave-instruction on gfx950,
// and sums must be deterministic).  The kernel takes srx_score_launch by value; score_block is the dispatch (open_item,
// one path per unit, emit_item); its own selections are srx_common.h's topk_cut; LDS that serves two purposes has a named
// accessor or a struct with its size assert (ScoreShared, FlatScratch).  DESIGN.md 4.2.

#include <stddef.h>

#include "srx_common.h"

namespace {

// LDS of one workgroup = one (query, split of the doc range) at a time
constexpr int RADIX8_BINS = 256;  // block_radix_kth_lds: 8-bit digits, one bin per thread
constexpr int OVF_CAP = 384;  // entries of the append scan's overflow area ((sizeof m_start + sizeof m_len) / 8)
struct ScoreShared {
    unsigned tbl[TBL_WORDS];  // hash keys [0,SLOTS) + vals [SLOTS,2*SLOTS)  |  dense acc[G]  |  radix hist
    TopkShared tk;
    int64_t m_start[MAXT];  // first posting of term i inside the current unit
    int m_len[MAXT];        // postings of term i inside the current unit
    float m_idf[MAXT];
    float m_qw[MAXT];
    unsigned short st_term[MAX_STEPS];  // step table of a hash unit: (term, first posting of the 256-chunk)
    int st_off[MAX_STEPS];
    int ptile[MAX_TPS + 1];  // overflow packer: postings per tile / group boundaries
    int grp[MAX_TPS + 1];
    int n_grp;
    unsigned ub_bits;  // srx_search_after: only candidates ranked strictly AFTER (ub_bits, ub_doc) in (score desc, doc asc)
    int ub_doc;        // order are collected; ub_bits = 0xFFFFFFFF: no bound (every score's bit pattern is below it)

    // ---- areas that borrow a table while its owner is idle ----
    // overflow area of the append scan: OVF_CAP (score bits, doc) entries on m_start / m_len (the wave-level dense path's runs travel in registers)
    __device__ __forceinline__ unsigned *ovf_bits() { return reinterpret_cast<unsigned *>(m_start); }
    __device__ __forceinline__ int *ovf_doc() { return reinterpret_cast<int *>(m_start) + OVF_CAP; }
    // histogram of block_radix_kth_lds (one bin per thread) on the hash path's step table, idle during a dense selection
    __device__ __forceinline__ unsigned *hist256() { return reinterpret_cast<unsigned *>(st_off); }
    static_assert(MAX_STEPS >= RADIX8_BINS && RADIX8_BINS == THREADS, "radix histogram on st_off, one bin per thread");
    // the private word a lane's masked postings are added to in the dense accumulation loops, on the same idle table
    __device__ __forceinline__ float *dummy_word(int lane) { return reinterpret_cast<float *>(st_off) + lane; }
    static_assert(MAX_STEPS >= 64, "dummy words on st_off: one per lane");
};
static_assert(offsetof(ScoreShared, m_len) == offsetof(ScoreShared, m_start) + sizeof(int64_t[MAXT]) &&
              sizeof(int64_t[MAXT]) + sizeof(int[MAXT]) >= OVF_CAP * 2 * sizeof(unsigned), "overflow area: m_len follows m_start, both hold it");

// srx_search_after's exclusive upper bound on (score bits, shard-local doc): true when the candidate ranks after it
// AFTER = false is the instance plain searches run: the test (two LDS reads + compares wherever a candidate is formed)
// measured 5.5 % of a C4 batch and 4 % of a C5 batch (profiles/r03_ab_tier2_after_bound.log).
template <bool AFTER>
__device__ __forceinline__ bool after_bound(const ScoreShared &S, unsigned b, int doc) {
    if constexpr (!AFTER) return true;
    return b < S.ub_bits || (b == S.ub_bits && doc > S.ub_doc);
}

// Hash-accumulate the unit described by m_start/m_len (P <= HASH_CAP postings) and fold its positive
// scores into the running top-k.  nt = terms in this pass.
// CP: the index dropped its canonical blocks -- postings come from the compact copy (16-bit local ids + ubase = the unit's
// first doc); every posting of a call then lies in ONE build unit (the host refuses unit overrides on such an index).
template <typename VT, bool AFTER, bool CP>
__device__ void hash_unit(ScoreShared &S, const IndexView &ix, int nt, int my_len, int k, int ubase) {
    const int tid = threadIdx.x;
    int *keys = reinterpret_cast<int *>(S.tbl);
    float *vals = reinterpret_cast<float *>(S.tbl + SLOTS);
    const int32_t *post = CP ? ix.post16 : ix.post;

    // step table: term i contributes ceil(len_i / 256) steps
    const unsigned my_chunks = (tid < nt) ? (unsigned)((my_len + THREADS - 1) / THREADS) : 0u;
    unsigned n_steps;
    const unsigned first = block_excl_scan(my_chunks, S.tk.red, &n_steps);
    for (unsigned c = 0; c < my_chunks; ++c) {
        S.st_term[first + c] = (unsigned short)tid;
        S.st_off[first + c] = (int)(c * THREADS);
    }
    __syncthreads();

    for (unsigned s0 = 0; s0 < n_steps; s0 += PREFETCH) {
        int d[PREFETCH];
        float v[PREFETCH];
#pragma unroll
        for (int r = 0; r < PREFETCH; ++r) {
            const unsigned s = s0 + r;
            d[r] = -1;
            v[r] = 0.f;
            if (s < n_steps) {
                const int i = S.st_term[s];
                const int p = S.st_off[s] + tid;
                if (p < S.m_len[i]) {
                    const int64_t g = S.m_start[i] + p;
                    d[r] = CP ? post16_doc_at<VT>(post, g, ubase) : post_doc_at<VT>(post, g);  // sentinels (run padding) read as negative docs: skipped below
                    v[r] = CP ? post16_val_at(post, g, VT()) : post_val_at(post, g, VT());
                }
            }
        }
#pragma unroll
        for (int r = 0; r < PREFETCH; ++r) {
            const unsigned s = s0 + r;
            if (s < n_steps) {
                const int i = S.st_term[s];
                if (s > 0 && S.st_term[s - 1] != i) __syncthreads();  // next term: order adds per doc
                if (d[r] >= 0) {
                    const float c = (v[r] * S.m_idf[i]) * S.m_qw[i];
                    unsigned h = ((unsigned)d[r] * 0x9E3779B1u) >> (32 - 13);
                    for (;;) {
                        const int old = atomicCAS(&keys[h], EMPTY_KEY, d[r]);
                        if (old == EMPTY_KEY) {
                            vals[h] = 0.0f + c;
                            break;
                        }
                        if (old == d[r]) {
                            vals[h] = vals[h] + c;
                            break;
                        }
                        h = (h + 1) & (SLOTS - 1);
                    }
                }
            }
        }
    }
    __syncthreads();
    // read the table into registers (4 consecutive slots per access), clear the keys behind us
    unsigned ubits[NPT_HASH];
    int udoc[NPT_HASH];
    const unsigned tau = S.tk.tau;
#pragma unroll
    for (int j = 0; j < NPT_HASH / 4; ++j) {
        const int q4 = j * THREADS + tid;
        const int4 kk = reinterpret_cast<const int4 *>(keys)[q4];
        const float4 vv = reinterpret_cast<const float4 *>(vals)[q4];
        reinterpret_cast<int4 *>(keys)[q4] = make_int4(EMPTY_KEY, EMPTY_KEY, EMPTY_KEY, EMPTY_KEY);
        const int ks[4] = {kk.x, kk.y, kk.z, kk.w};
        const float vs[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const unsigned b = __float_as_uint(vs[c]);
            const bool ok = ks[c] != EMPTY_KEY && vs[c] > 0.0f && b >= tau && after_bound<AFTER>(S, b, ks[c]);
            ubits[j * 4 + c] = ok ? b : 0u;
            udoc[j * 4 + c] = ks[c];
        }
    }
    __syncthreads();  // table is free from here: vals region doubles as the radix histogram
    topk_fold<NPT_HASH, true>(ubits, udoc, k, S.tk, S.tbl + SLOTS);
}

// Dense-accumulate one tile of G docs [tile_base, tile_base + G) described by m_start/m_len.
// first_pass: zero the accumulators; last_pass: select.  (Queries with > MAXT terms take several passes.)
template <typename VT, bool CP>
__device__ void dense_tile_accumulate(ScoreShared &S, const IndexView &ix, int nt, int tile_base, bool first_pass, int ubase) {
    const int tid = threadIdx.x;
    float *acc = reinterpret_cast<float *>(S.tbl);
    const int G = 1 << ix.tile_log2;
    const int32_t *post = CP ? ix.post16 : ix.post;
    constexpr int BW = CP ? CompactWords<VT>::value : BlockWords<VT>::value;
    if (first_pass) {
        for (int i = tid; i < G / 4; i += THREADS) reinterpret_cast<float4 *>(acc)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        __syncthreads();
    }
    // Batches of 2048 postings (two stripes of whole blocks = 8 postings per thread) are enumerated term-major; a ring
    // of K = 4 batches is in flight, across term boundaries too, so a term's load latency hides behind the
    // previous terms' work (one batch ahead left the dense tiles latency-bound).  A barrier separates consecutive
    // batches of different terms (the next term may touch the same doc).  A tile's run [start, start + len) starts at
    // an arbitrary padded position: the batches cover the blocks from start & ~3 on, postings outside the run and
    // sentinels (doc -1) are blanked.
    constexpr int NB = 8;                 // postings per thread per batch (whole blocks of 4)
    constexpr int BATCH = THREADS * NB;
    auto next_term = [&](int i) {  // first term index >= i with postings in this tile (uniform), nt if none
        while (i < nt && S.m_len[i] == 0) ++i;
        return i;
    };
    auto span_of = [&](int i) { return (int)(S.m_start[i] & 3) + S.m_len[i]; };  // postings from the first block's start
    auto load_batch = [&](int i_, int o, int (&d)[NB], float (&v)[NB]) {
        const bool valid = i_ < nt;        // past the last batch: the loads are still issued (a constant number in flight ->
        const int i = valid ? i_ : 0;      // counted vmcnt waits), everything masked
        const int64_t start = S.m_start[i];
        const int head = (int)(start & 3);
        const int span = valid ? head + S.m_len[i] : 0;
        const int64_t b0 = start >> 2;
#pragma unroll
        for (int h = 0; h < NB / 4; ++h) {
            const int p = o + h * (THREADS * 4) + tid * 4;  // my block of this stripe, in postings from the first block
            const int64_t blk = (p < span) ? b0 + (p >> 2) : b0;  // idle threads re-read the run's first block (always valid)
            int dd[4];
            float vv[4];
            if constexpr (CP)
                load_block16(post + blk * BW, VT(), dd, vv);  // unit-local ids
            else
                load_block(post + blk * BW, VT(), dd, vv);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                // CP: d = the accumulator index inside the tile (local id - the tile's offset in its unit); a sentinel's
                // (local id >= 49152) lies outside [0, G) for every tile of a unit and is skipped by add_batch
                const int dc = CP ? dd[c] - (tile_base - ubase) : dd[c];
                d[4 * h + c] = (p + c >= head && p + c < span) ? dc : -1;
                v[4 * h + c] = vv[c];
            }
        }
    };
    auto add_batch = [&](int i, const int (&d)[NB], const float (&v)[NB]) {
        const float idf = S.m_idf[i], qw = S.m_qw[i];
        // The postings of one batch belong to one term, so their docs are distinct: read all accumulators, then write
        // them all (written as one loop of read-modify-writes the compiler has to assume the addresses may alias and
        // serialises NB LDS round trips per batch -- the dense tiles' main stall before).
        // Branch-free: a masked posting (doc < 0) reads and writes a private dummy word instead of an accumulator (as
        // per-posting branches the compiler emitted one exec-masked block and one LDS wait per posting).
        float *const dummy = S.dummy_word(tid & 63);
        float *slot[NB];
        float acc_r[NB];
#pragma unroll
        for (int r = 0; r < NB; ++r)
            slot[r] = CP ? (((unsigned)d[r] < (unsigned)G) ? acc + d[r] : dummy) : ((d[r] >= 0) ? acc + (d[r] - tile_base) : dummy);
#pragma unroll
        for (int r = 0; r < NB; ++r) acc_r[r] = *slot[r];
#pragma unroll
        for (int r = 0; r < NB; ++r) *slot[r] = acc_r[r] + (v[r] * idf) * qw;
    };
    // K batches in flight: register set j holds batch n with n % K == j; after batch n has been accumulated its set is
    // refilled with batch n + K.  (One batch ahead left a many-term tile -- 50 terms of < 1 batch each -- paying one full
    // memory round trip per term: profiles/r02_c4_*.)
    constexpr int K = 4;
    int qi[K], qo[K];  // term / offset of the batch in set j (qi == nt: none)
    int dq[K][NB];
    float vq[K][NB];
    int ni = next_term(0), no = 0;  // the next batch to load
    auto advance = [&]() {          // (ni, no) -> its successor in term-major order
        no += BATCH;
        if (no >= span_of(ni)) {
            ni = next_term(ni + 1);
            no = 0;
        }
    };
    if (ni >= nt) return;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        qi[j] = ni;
        qo[j] = no;
        load_batch(ni, no, dq[j], vq[j]);
        if (ni < nt) advance();
    }
    while (qi[0] < nt) {  // set 0 holds the oldest batch at the top of the loop
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (qi[j] < nt) add_batch(qi[j], dq[j], vq[j]);  // uniform
            const int nxt = qi[(j + 1) % K];  // term of the batch that is accumulated next
            if (qi[j] < nt && nxt < nt && nxt != qi[j]) __syncthreads();  // next term: order the adds per doc
            qi[j] = ni;
            qo[j] = no;
            load_batch(ni, no, dq[j], vq[j]);
            if (ni < nt) advance();
        }
    }
    __syncthreads();
}

// One tile (<= 2^14 docs) holding P <= FLAT_CAP postings of MANY terms (learned-sparse queries: 50 terms with ~80
// postings each), all terms at once instead of term by term with a barrier and a memory round trip per term:
//   1. every posting sets its doc's bit in an LDS bitmap; a bit found set marks the doc in a second bitmap (multi-term);
//   2. second pass (postings come from L1/L2 now): a posting of a single-term doc is the doc's whole score (0 + c) and
//      becomes a candidate directly; postings of multi-term docs (a few %) go to an LDS list;
//   3. the list is grouped by doc (hash claim + count + scan + scatter) and each doc's contributions are added in
//      ascending term order by one thread -- the reference's accumulation order, exactly;
//   4. singles and multis are folded into the block's running top-k.
// Returns false (nothing folded, LDS scratch only) when more than FLAT_MCAP postings belong to multi-term docs: the
// caller then uses the dense accumulators.
constexpr int FLAT_CAP = 8192;                 // postings per flat tile (32 per thread)
constexpr int FLAT_NPT = FLAT_CAP / THREADS;
constexpr int FLAT_MCAP = 2048;                // multi-term postings per flat tile
constexpr int FLAT_SLOTS = 2048;               // doc hash slots of the grouping step (>= 2 x docs: a multi doc has >= 2 postings)
constexpr int FLAT_MPT = FLAT_MCAP / THREADS;  // 8
constexpr int FLAT_MIN_TERMS = 12;             // below this the term-by-term paths are at least as good

constexpr int FLAT_HDR = TBL_WORDS - 4 * FLAT_MCAP - 3 * FLAT_SLOTS;  // flat_tile's scratch, laid over the 64 KiB table: words before mk_key
struct FlatScratch {
    unsigned bm1[MAX_G / 32], bm2[MAX_G / 32];  // doc seen / doc seen twice: one bit per doc of the tile
    int pre[MAXT + 1];                          // exclusive prefix of m_len: flat posting index -> term
    unsigned mcount;                            // multi-term postings collected
    unsigned pad_[FLAT_HDR - (2 * (MAX_G / 32) + MAXT + 2)];  // the header takes what the arrays below leave of the table
    int mk_key[FLAT_MCAP];                      // the multi-term postings: (doc << 8 | term, contribution) ...
    float mk_c[FLAT_MCAP];
    int so_key[FLAT_MCAP];                      // ... and the same grouped by doc
    float so_c[FLAT_MCAP];
    int hk[FLAT_SLOTS], hcnt[FLAT_SLOTS], hoff[FLAT_SLOTS];  // doc hash of the grouping step: key, postings, first position
};
static_assert(sizeof(FlatScratch) == sizeof(unsigned[TBL_WORDS]) && offsetof(FlatScratch, mk_key) == FLAT_HDR * 4, "flat_tile scratch fills the table exactly");
static_assert(2 * (MAX_G / 32) == 4 * THREADS && MAXT <= 256, "one uint4 per thread zeroes both bitmaps; mk_key / so_key pack the term into 8 bits");

template <typename VT, bool AFTER, bool CP>
__device__ bool flat_tile(ScoreShared &S, const IndexView &ix, int nt, int my_len, int tile_base, int k) {  // one-tile units: the tile IS the unit
    const int tid = threadIdx.x;
    FlatScratch &F = *reinterpret_cast<FlatScratch *>(S.tbl);
    unsigned *bm1 = F.bm1, *bm2 = F.bm2, *mcount = &F.mcount;
    int *pre = F.pre, *mk_key = F.mk_key, *so_key = F.so_key, *hk = F.hk, *hcnt = F.hcnt, *hoff = F.hoff;
    float *mk_c = F.mk_c, *so_c = F.so_c;
    const int32_t *post = CP ? ix.post16 : ix.post;

    unsigned P;
    const unsigned first = block_excl_scan(tid < nt ? (unsigned)my_len : 0u, S.tk.red, &P);
    if (tid < nt) pre[tid] = (int)first;
    if (tid == 0) {
        pre[nt] = (int)P;
        *mcount = 0;
    }
    reinterpret_cast<uint4 *>(F.bm1)[tid] = make_uint4(0u, 0u, 0u, 0u);  // both bitmaps
    for (int i = tid; i < FLAT_SLOTS; i += THREADS) {
        hk[i] = EMPTY_KEY;
        hcnt[i] = 0;
    }
    __syncthreads();
    // ---- 1. mark ----
    {
        int i = 0;
        for (int f = tid; f < (int)P; f += THREADS) {
            while (f >= pre[i + 1]) ++i;
            const int da = CP ? post16_doc_at<VT>(post, S.m_start[i] + (f - pre[i]), tile_base) : post_doc_at<VT>(post, S.m_start[i] + (f - pre[i]));
            if (da >= 0) {  // not a sentinel
                const int d = da - tile_base;
                const unsigned bit = 1u << (d & 31);
                if (atomicOr(&bm1[d >> 5], bit) & bit) atomicOr(&bm2[d >> 5], bit);
            }
        }
    }
    __syncthreads();
    // ---- 2. classify: singles to registers, multi postings to the list ----
    unsigned ubits[FLAT_NPT];
    int udoc[FLAT_NPT];
    const unsigned tau = S.tk.tau;
    {
        int i = 0;
#pragma unroll
        for (int n = 0; n < FLAT_NPT; ++n) {
            const int f = n * THREADS + tid;
            ubits[n] = 0u;
            udoc[n] = 0;
            if (f < (int)P) {
                while (f >= pre[i + 1]) ++i;
                const int64_t g = S.m_start[i] + (f - pre[i]);
                const int da = CP ? post16_doc_at<VT>(post, g, tile_base) : post_doc_at<VT>(post, g);
                const int d = da - tile_base;
                const float c = ((CP ? post16_val_at(post, g, VT()) : post_val_at(post, g, VT())) * S.m_idf[i]) * S.m_qw[i];
                if (da < 0) {  // sentinel: nothing
                } else if ((bm2[d >> 5] >> (d & 31)) & 1u) {
                    const unsigned e = atomicAdd(mcount, 1u);
                    if (e < (unsigned)FLAT_MCAP) {
                        mk_key[e] = (d << 8) | i;
                        mk_c[e] = c;
                    }
                } else {
                    const float sc = 0.0f + c;
                    const unsigned b = __float_as_uint(sc);
                    if (sc > 0.0f && b >= tau && after_bound<AFTER>(S, b, tile_base + d)) {
                        ubits[n] = b;
                        udoc[n] = tile_base + d;
                    }
                }
            }
        }
    }
    __syncthreads();
    const unsigned M = *mcount;
    if (M > (unsigned)FLAT_MCAP) return false;  // uniform
    // ---- 3. group the multi postings by doc ----
    int slot[FLAT_MPT];
#pragma unroll
    for (int j = 0; j < FLAT_MPT; ++j) {
        const unsigned e = j * THREADS + tid;
        slot[j] = -1;
        if (e < M) {
            const int d = mk_key[e] >> 8;
            unsigned h = ((unsigned)d * 0x9E3779B1u) >> (32 - 11);
            for (;;) {
                const int old = atomicCAS(&hk[h], EMPTY_KEY, d);
                if (old == EMPTY_KEY || old == d) break;
                h = (h + 1) & (FLAT_SLOTS - 1);
            }
            slot[j] = (int)h;
            atomicAdd(&hcnt[h], 1);
        }
    }
    __syncthreads();
    {
        constexpr int SPT = FLAT_SLOTS / THREADS;  // 8 consecutive slots per thread
        int c8[SPT];
        unsigned mine = 0;
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            c8[j] = hcnt[tid * SPT + j];
            mine += (unsigned)c8[j];
        }
        unsigned tot;
        unsigned run = block_excl_scan(mine, S.tk.red, &tot);
#pragma unroll
        for (int j = 0; j < SPT; ++j) {
            hoff[tid * SPT + j] = (int)run;
            run += (unsigned)c8[j];
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < FLAT_MPT; ++j) {
        if (slot[j] >= 0) {
            const unsigned e = j * THREADS + tid;
            const int pos = hoff[slot[j]] + atomicSub(&hcnt[slot[j]], 1) - 1;
            so_key[pos] = mk_key[e];
            so_c[pos] = mk_c[e];
        }
    }
    __syncthreads();
    // one thread per doc slot: contributions in ascending term order
    unsigned mbits[FLAT_MPT];
    int mdoc[FLAT_MPT];
#pragma unroll
    for (int j = 0; j < FLAT_MPT; ++j) {
        const int sl = tid * FLAT_MPT + j;
        const int a = hoff[sl];
        const int b = (sl + 1 < FLAT_SLOTS) ? hoff[sl + 1] : (int)M;
        mbits[j] = 0u;
        mdoc[j] = 0;
        if (b > a) {
            float sum = 0.0f;
            int last = -1;
            for (int n = a; n < b; ++n) {  // selection by term: b - a is 2 or 3 almost always
                int best = 0x7FFFFFFF, bi = a;
                for (int m = a; m < b; ++m) {
                    const int t = so_key[m] & 0xFF;
                    if (t > last && t < best) {
                        best = t;
                        bi = m;
                    }
                }
                sum = sum + so_c[bi];
                last = best;
            }
            const unsigned bb = __float_as_uint(sum);
            if (sum > 0.0f && bb >= tau && after_bound<AFTER>(S, bb, tile_base + (so_key[a] >> 8))) {
                mbits[j] = bb;
                mdoc[j] = tile_base + (so_key[a] >> 8);
            }
        }
    }
    __syncthreads();  // the scratch is free from here: it doubles as the radix histogram of the folds
    topk_fold<FLAT_NPT, true>(ubits, udoc, k, S.tk, S.tbl);
    topk_fold<FLAT_MPT, true>(mbits, mdoc, k, S.tk, S.tbl);
    return true;
}

// Dense accumulation of ONE tile by ONE wavefront (tiles of <= 4096 docs: four waves' accumulators fit the 64 KiB table,
// so a workgroup takes four consecutive tiles at a time).  No block barrier anywhere: the wave streams the tile's runs
// term by term in the query's term order and one wave's LDS instructions execute in order, which is all the per-doc
// summation order needs.  Lane i < nt carries term i's run in this tile (wstart / wlen) and its weights (my_idf /
// my_qw); K blocks per lane are in flight across term boundaries.  The block kernel's term-by-term form costs a barrier
// and a memory round trip per term: on 50-term learned-sparse queries (C4) that was 85 % of its time.
// ALIGNED (the index has one-tile units: every run of a tile starts on a block boundary and ends in sentinels): only the
// sentinel test is left of the masks, idle lanes read their own all-sentinel block.
// (Measured and dropped: adding with the LDS float atomic ds_add_f32 instead of read / add / write.  It is bit-identical
// to v_add_f32 and ordered -- tools/lds_fadd_probe.hip -- and needs half the instructions, but the LDS executes it at
// about one lane every 7 cycles: C4 went from 47 ms to 166 ms per batch.)
// (Measured and dropped: reading the compact copy of srx_common.h here on one-tile units -- a local id IS the accumulator
// index, one 16-byte load per fp16 block instead of 16 + 8.  C4: 21.7 -> 20.8 ms per batch for 33 % fewer bytes: the path
// is bound by its LDS round trips, not by HBM, so the second copy's traffic saving buys little.)
template <typename VT, bool ALIGNED, bool CP>
__device__ void wave_dense_accumulate(ScoreShared &S, const IndexView &ix, int nt, int64_t tile_base, bool has_tile, int64_t wstart,
                                      int wlen, float my_idf, float my_qw) {
    constexpr int BW = CP ? CompactWords<VT>::value : BlockWords<VT>::value;
    const int ubase = (int)((((tile_base >> ix.tile_log2) / ix.unit_tiles) * ix.unit_tiles) << ix.tile_log2);  // first doc of the tile's build unit
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int G = 1 << ix.tile_log2;
    float *acc = reinterpret_cast<float *>(S.tbl) + wave * G;
    for (int i = lane; i < G / 4; i += 64) reinterpret_cast<float4 *>(acc)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!has_tile) return;  // uniform per wave
    const int32_t *post = CP ? ix.post16 : ix.post;
    const int64_t idle_blk = ix.zero_block + lane;  // my all-sentinel block
    // iterator over (term, step): 64 blocks per step
    int it = 0, istep = 0;       // next (term, step) to load
    int64_t cs = 0;              // its run start / length (uniform)
    int cl = 0, cnb = 0;
    auto seek = [&]() {          // make (it, istep) point at an existing step, or it = nt
        for (;;) {
            if (it >= nt) return;
            if (istep == 0) {
                cs = ((int64_t)__builtin_amdgcn_readlane((int)(wstart >> 32), it) << 32) |
                     (unsigned)__builtin_amdgcn_readlane((int)(wstart & 0xFFFFFFFFll), it);
                cl = __builtin_amdgcn_readlane(wlen, it);
                cnb = cl > 0 ? (int)(((cs & 3) + cl + 3) >> 2) : 0;
            }
            if (istep * 64 < cnb) return;
            ++it;
            istep = 0;
        }
    };
    struct Blk {
        int d[4];
        float v[4];
        float idf, qw;  // uniform
    };
    // Loads the block of (it, istep) for this lane and advances the iterator.  ALWAYS issues its loads (past the end: an
    // all-sentinel block), so that the number of loads in flight is a compile-time constant and the waits before the adds
    // are counted vmcnt waits, not vmcnt(0).
    auto load = [&](Blk &b) {
        const bool valid = it < nt;
        const int t = valid ? it : 0;
        b.idf = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(my_idf), t));
        b.qw = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(my_qw), t));
        const int bi = istep * 64 + lane;
        const bool ok = valid && bi < cnb;
        int dd[4];
        float vv[4];
        if constexpr (CP)
            load_block16(post + (ok ? (cs >> 2) + bi : idle_blk) * BW, VT(), dd, vv);  // unit-local ids; a sentinel's (>= 49152) is no
        else                                                                           // accumulator index of any tile
            load_block(post + (ok ? (cs >> 2) + bi : idle_blk) * BW, VT(), dd, vv);
        const int head = (int)(cs & 3), span = head + cl;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int p = bi * 4 + c;
            // CP: b.d = the accumulator index inside the tile (local id - the tile's offset in its unit: 0 on one-tile units);
            // anything outside [0, G) is skipped by add()
            const int dc = CP ? dd[c] - (int)(tile_base - ubase) : dd[c];
            b.d[c] = (ALIGNED || (ok && p >= head && p < span)) ? dc : -1;
            b.v[c] = vv[c];
        }
        if (valid) ++istep;
    };
    // branch-free: a masked posting / sentinel (doc < 0) goes to a private dummy word; one term's docs are distinct
    float *const dummy = S.dummy_word(lane);
    float *const acc0 = acc - (int)tile_base;
    auto add = [&](const Blk &b) {
        float *slot[4];
        float a[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            slot[c] = CP ? (((unsigned)b.d[c] < (unsigned)G) ? acc + b.d[c] : dummy) : ((b.d[c] >= 0) ? acc0 + b.d[c] : dummy);
#pragma unroll
        for (int c = 0; c < 4; ++c) a[c] = *slot[c];
#pragma unroll
        for (int c = 0; c < 4; ++c) *slot[c] = a[c] + (b.v[c] * b.idf) * b.qw;
    };
    constexpr int K = 4;  // blocks in flight per lane
    Blk q[K];
    bool live[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
        seek();
        live[j] = it < nt;
        load(q[j]);
    }
    while (live[0]) {  // set 0 always holds the oldest block at the top of the loop
#pragma unroll
        for (int j = 0; j < K; ++j) {
            add(q[j]);  // a dead set holds sentinels / masked postings only: nothing is added
            seek();
            live[j] = it < nt;
            load(q[j]);
        }
    }
}

// Exact k-th largest over n_items keys that STAY IN LDS (keyfn(i) re-reads them in every pass; key 0 = none, keys in
// [1, 2^31)): MSD radix select with 8-bit digits, one histogram bin per thread (hist = 256 words).  The block-level
// sibling of wave_radix_kth: no per-thread key arrays, so nothing spills (the register-array form radix_kth<N> cost the
// dense tiles ~500 bytes of scratch per lane and as many HBM bytes as the postings themselves: profiles/r02_c5_*).
// Requires 1 <= k <= #candidates; mx / mn = max / min candidate key.  Returns T; n_gt = #keys > T, n_eq = #keys == T.
template <typename KeyFn>
__device__ unsigned block_radix_kth_lds(KeyFn keyfn, unsigned n_items, unsigned k, unsigned mx, unsigned mn, unsigned n_cand,
                                        unsigned *hist, unsigned *red, unsigned *n_gt, unsigned *n_eq) {
    if (mx == mn) {
        *n_gt = 0;
        *n_eq = n_cand;
        return mx;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hb = 31 - __clz(mx ^ mn);
    unsigned prefix = mx & ~((2u << hb) - 1u);
    int shift = hb + 1;
    unsigned krem = k, gt = 0, eq = 0;
    while (shift > 0) {
        const int w = shift < 8 ? shift : 8;
        shift -= w;
        const int hi_shift = shift + w;
        hist[tid] = 0;
        __syncthreads();
        for (unsigned i = tid; i < n_items; i += THREADS) {
            const unsigned x = keyfn(i);
            if (x != 0 && ((x ^ prefix) >> hi_shift) == 0) atomicAdd(&hist[(x >> shift) & ((1u << w) - 1u)], 1u);
        }
        __syncthreads();
        const unsigned sb = hist[tid];
        unsigned suf = sb;  // inclusive suffix sum over threads >= tid
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned v = __shfl_down(suf, o);
            if (lane + o < 64) suf += v;
        }
        if (lane == 0) red[wave] = suf;
        __syncthreads();
#pragma unroll
        for (int ww = 0; ww < WAVES; ++ww)
            if (ww > wave) suf += red[ww];
        const unsigned above = suf - sb;
        if (above < krem && krem <= suf) {
            red[8] = (unsigned)tid;
            red[9] = above;
            red[10] = sb;
        }
        __syncthreads();
        const unsigned d = red[8], ab = red[9];
        eq = red[10];
        krem -= ab;
        gt += ab;
        prefix |= d << shift;
        __syncthreads();
    }
    *n_gt = gt;
    *n_eq = eq;
    return prefix;
}

// Running list + overflow area -> the k best, tau = the k-th best.  n_total = entries appended so far: positions
// [0, KMAX) live in tk.bits / tk.doc, [KMAX, KMAX + OVF_CAP) in the overflow area.  Requires k <= n_total <=
// KMAX + OVF_CAP and k <= KMAX.  Every entry is a real candidate (key >= 1).  Touches ~1.4 k entries instead of the
// tile's 16 k accumulators (dense_tile_general).
__device__ void list_compact_select(ScoreShared &S, int k, unsigned n_total) {
    const int tid = threadIdx.x;
    auto key1 = [&](unsigned i) -> unsigned { return i < (unsigned)KMAX ? S.tk.bits[i] : S.ovf_bits()[i - KMAX]; };
    auto doc_of = [&](unsigned i) -> int { return i < (unsigned)KMAX ? S.tk.doc[i] : S.ovf_doc()[i - KMAX]; };
    constexpr int IPT = (KMAX + OVF_CAP + THREADS - 1) / THREADS;  // entries per thread
    unsigned ek[IPT];
    int ed[IPT];
#pragma unroll
    for (int j = 0; j < IPT; ++j) {
        const unsigned i = tid + j * THREADS;
        ek[j] = i < n_total ? key1(i) : 0u;
        ed[j] = i < n_total ? doc_of(i) : 0;
    }
    const TopkCut cut = topk_cut((unsigned)k, n_total, [&](auto keys, unsigned kk, unsigned n_cand, unsigned *n_gt, unsigned *n_eq) {
        unsigned mx = 0, mn = 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const unsigned x = keys(ek[j], ed[j]);
            if (x != 0u) {
                mx = max(mx, x);
                mn = min(mn, x);
            }
        }
        const SumMaxMin r = block_sum_max_min(0u, mx, mn, S.tk.red);
        return block_radix_kth_lds([&](unsigned i) -> unsigned { return keys(key1(i), doc_of(i)); }, n_total, kk, r.mx, r.mn, n_cand,
                                   S.hist256(), S.tk.red, n_gt, n_eq);
    });
    __syncthreads();  // every read of the old entries is done (the registers hold them)
    if (tid == 0) {
        S.tk.count = 0;
        S.tk.tau = cut.T;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < IPT; ++j)
        if (cut.keeps(ek[j], ed[j])) list_push(S.tk, ek[j], ed[j]);
    __syncthreads();
}

// The append scan of a dense tile: one pass over the accumulators (G = span_tiles << tile_log2 of them, in LDS) appends
// every candidate to the lazy list and, past its capacity KMAX, to the first ovf_cap entries of the overflow area (0 where
// m_start / m_len are live).  n_old = tk.count as the caller read it BEFORE its last barrier.  Returns true when the tile is
// served: no selection ran; the caller shrinks a list that reaches into the overflow area back into tk (list_compact_select)
// before anything else reads it.  When the appends do not fit they are dropped, what was there before is shrunk to its k
// best (tau rises) and the scan runs once more.  Still too many (a query's first tiles), or nothing to shrink: false, the
// list is what it was (or its k best) and dense_tile_general has to serve the tile.
template <bool AFTER>
__device__ bool dense_tile_append(ScoreShared &S, const IndexView &ix, int tile_base, int k, int span_tiles, unsigned n_old, int ovf_cap) {
    const int tid = threadIdx.x, lane = tid & 63;
    const float *acc = reinterpret_cast<const float *>(S.tbl);
    const int G = span_tiles << ix.tile_log2;
    unsigned *ovf_bits = S.ovf_bits();
    int *ovf_doc = S.ovf_doc();
    for (int attempt = 0; attempt < 2; ++attempt) {
        const unsigned tau_now = S.tk.tau;
        // accumulators of docs past n_docs were zeroed and never touched: no bound check.  G / 4 is a multiple of
        // THREADS (whole waves run every iteration); four float4 per thread are read before anything is tested
        auto append4 = [&](int i, const float4 a4) {  // whole waves only
            const float a[4] = {a4.x, a4.y, a4.z, a4.w};
            bool ok[4];
            unsigned long long m[4];
            unsigned tot = 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                ok[c] = a[c] > 0.0f && __float_as_uint(a[c]) >= tau_now && after_bound<AFTER>(S, __float_as_uint(a[c]), tile_base + 4 * i + c);
                m[c] = __ballot(ok[c]);
                tot += (unsigned)__popcll(m[c]);
            }
            if (tot == 0u) return;  // uniform
            unsigned base = 0;      // one atomic per wave; a candidate's slot = its rank among the wave's candidates
            if (lane == 0) base = atomicAdd(&S.tk.count, tot);
            base = (unsigned)__builtin_amdgcn_readfirstlane((int)base);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (ok[c]) {
                    const unsigned p = base + __builtin_amdgcn_mbcnt_hi((unsigned)(m[c] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m[c], 0u));
                    if (p < (unsigned)KMAX) {
                        S.tk.bits[p] = __float_as_uint(a[c]);
                        S.tk.doc[p] = tile_base + 4 * i + c;
                    } else if (p < (unsigned)(KMAX + ovf_cap)) {
                        ovf_bits[p - KMAX] = __float_as_uint(a[c]);
                        ovf_doc[p - KMAX] = tile_base + 4 * i + c;
                    }
                }
                base += (unsigned)__popcll(m[c]);
            }
        };
        // signed-int order of the bit patterns = float order for x > 0, negatives sort below: a conservative screen
        const int tau_i = (int)max(tau_now, 1u);
        const float4 *acc4 = reinterpret_cast<const float4 *>(acc);
        auto imax4 = [](const float4 r) {
            return max(max(__float_as_int(r.x), __float_as_int(r.y)), max(__float_as_int(r.z), __float_as_int(r.w)));
        };
        const int n4 = G / 4, n4r = (n4 + 63) & ~63;  // whole waves run every iteration (tiny tiles: n4 < 64)
        const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
        int i = tid;
        for (; i + 3 * THREADS < n4; i += 4 * THREADS) {
            const float4 r0 = acc4[i], r1 = acc4[i + THREADS], r2 = acc4[i + 2 * THREADS], r3 = acc4[i + 3 * THREADS];
            const int mm = max(max(imax4(r0), imax4(r1)), max(imax4(r2), imax4(r3)));
            // no accumulator of these 16 x 64 can enter: the common case once tau has risen
            if (__ballot(mm >= tau_i) == 0ull) continue;
            append4(i, r0);
            append4(i + THREADS, r1);
            append4(i + 2 * THREADS, r2);
            append4(i + 3 * THREADS, r3);
        }
        for (; i < n4r; i += THREADS) append4(i, i < n4 ? acc4[i] : zero4);
        __syncthreads();
        const unsigned n_total = S.tk.count;
        if (n_total <= (unsigned)(KMAX + ovf_cap)) return true;  // uniform.  The list stays lazy: no selection until it is full
        __syncthreads();
        if (tid == 0) S.tk.count = n_old;
        __syncthreads();
        if (n_old <= (unsigned)k) break;
        list_compact_select(S, k, n_old);
        n_old = (unsigned)k;
    }
    return false;
}

// The general selection of a dense tile: a counting pass over the accumulators, then either an append pass (the lazy list
// has room) or the exact cut over (list U tile candidates), whose keys are re-read from LDS in every radix pass.
template <bool AFTER>
__device__ void dense_tile_general(ScoreShared &S, const IndexView &ix, int tile_base, int k, int span_tiles) {
    const int tid = threadIdx.x;
    const float *acc = reinterpret_cast<const float *>(S.tbl);
    const int G = span_tiles << ix.tile_log2;  // accumulators in LDS: span_tiles consecutive tiles
    const unsigned tau = S.tk.tau;
    const unsigned n_old = S.tk.count;  // read BEFORE the barriers below
    const int n_valid = (int)min((int64_t)G, ix.n_docs - (int64_t)tile_base);  // docs of this tile that exist
    auto cand_key = [&](int o) -> unsigned {  // key of accumulator o: its score bits when it can enter the list, else 0
        const float x = acc[o];
        const unsigned b = __float_as_uint(x);
        return (x > 0.0f && b >= tau && after_bound<AFTER>(S, b, tile_base + o)) ? b : 0u;
    };
    unsigned mine = 0, lmx = 0, lmn = 0xFFFFFFFFu;
    for (int o = tid; o < n_valid; o += THREADS) {
        const unsigned x = cand_key(o);
        if (x != 0u) {
            ++mine;
            lmx = max(lmx, x);
            lmn = min(lmn, x);
        }
    }
    const SumMaxMin r = block_sum_max_min(mine, lmx, lmn, S.tk.red);
    const unsigned n_new = r.sum;
    if (n_new == 0 && n_old <= (unsigned)k) return;  // uniform
    if (n_old + n_new <= (unsigned)KMAX) {  // room in the lazy list: append
        for (int o = tid; o < n_valid; o += THREADS) {
            const unsigned x = cand_key(o);
            if (x != 0u) list_push(S.tk, x, tile_base + o);
        }
        __syncthreads();
        return;
    }
    // ---- the cut over (list U candidates) ----
    unsigned omx = 0, omn = 0xFFFFFFFFu;
    for (unsigned i = tid; i < n_old; i += THREADS) {
        omx = max(omx, S.tk.bits[i]);
        omn = min(omn, S.tk.bits[i]);
    }
    const unsigned n_items = n_old + (unsigned)n_valid;
    auto key1 = [&](unsigned i) -> unsigned { return i < n_old ? S.tk.bits[i] : cand_key((int)(i - n_old)); };
    auto doc_of = [&](unsigned i) -> int { return i < n_old ? S.tk.doc[i] : tile_base + (int)(i - n_old); };
    const TopkCut cut = topk_cut((unsigned)k, n_old + n_new, [&](auto keys, unsigned kk, unsigned n_cand, unsigned *n_gt, unsigned *n_eq) {
        auto key = [&](unsigned i) -> unsigned { return keys(key1(i), doc_of(i)); };
        unsigned mx = max(omx, r.mx), mn = min(omn, r.mn);  // the score keys: the list's range and the counting pass's
        if constexpr (!decltype(keys)::SCORE) {
            mx = 0;
            mn = 0xFFFFFFFFu;
            for (unsigned i = tid; i < n_items; i += THREADS) {
                const unsigned x = key(i);
                if (x != 0u) {
                    mx = max(mx, x);
                    mn = min(mn, x);
                }
            }
        }
        const SumMaxMin rr = block_sum_max_min(0u, mx, mn, S.tk.red);
        return block_radix_kth_lds(key, n_items, kk, rr.mx, rr.mn, n_cand, S.hist256(), S.tk.red, n_gt, n_eq);
    });
    // rebuild the list: the old entries first go to registers (KPT per thread), then everything that survives is appended
    unsigned okey[KPT];
    int odoc[KPT];
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
        const unsigned i = tid + j * THREADS;
        okey[j] = i < n_old ? S.tk.bits[i] : 0u;
        odoc[j] = i < n_old ? S.tk.doc[i] : 0;
    }
    __syncthreads();
    if (tid == 0) {
        S.tk.count = 0;
        S.tk.tau = cut.T;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < KPT; ++j)
        if (cut.keeps(okey[j], odoc[j])) list_push(S.tk, okey[j], odoc[j]);
    // candidates below the OLD tau were already excluded by cand_key (tau captured above); T >= that tau
    for (int o = tid; o < n_valid; o += THREADS) {
        const unsigned x = cand_key(o);
        if (cut.keeps(x, tile_base + o)) list_push(S.tk, x, tile_base + o);
    }
    __syncthreads();
}

constexpr int DENSE_MIN = HASH_CAP;  // a tile with more postings than this is accumulated densely

// thread i < nt: term i's run in the unit that hash_unit / flat_tile / dense_tile_accumulate read after the caller's barrier
__device__ __forceinline__ void set_runs(ScoreShared &S, int nt, int64_t start, int len) {
    if ((int)threadIdx.x < nt) {
        S.m_start[threadIdx.x] = start;
        S.m_len[threadIdx.x] = len;
    }
}

// Back to hash mode: the key half of the table reads as empty (dense accumulators or flat_tile's scratch were there).
__device__ __forceinline__ void hash_mode(ScoreShared &S) {
    int *keys = reinterpret_cast<int *>(S.tbl);
    for (int i = threadIdx.x; i < SLOTS; i += THREADS) keys[i] = EMPTY_KEY;
    __syncthreads();
}

// Opens a work item: empty list, the search-after bound, the table in hash mode, and the initial threshold from the
// index's per-term score bounds (see srx_wave_kernel): an exact lower bound on the k-th best score when every query idf is
// >= 0.  Returns true when a weight of the query is inf / nan.
__device__ bool open_item(ScoreShared &S, const srx_score_launch &a, int q, int t0, int nt_all) {
    const int tid = threadIdx.x;
    const IndexView &ix = a.w.ix;
    const int col = bound_column(a.w.k);
    unsigned t0b = 0, negf = 0;
    for (int i = tid; i < nt_all; i += THREADS) {
        const int term = a.w.q_term[t0 + i];
        const float idf = ix.idf[term], qw = a.w.q_weight[t0 + i];
        if (!(fabsf(idf) <= 3.0e38f) || !(fabsf(qw) <= 3.0e38f)) negf |= 0x10000u;  // inf / nan weight
        if (idf < 0.0f || qw < 0.0f) {
            negf |= 1u;
        } else if (ix.term_bound != nullptr && col >= 0 && idf > 0.0f && qw > 0.0f) {
            const float b = 0.0f + (ix.term_bound[(int64_t)term * 4 + col] * idf) * qw;
            t0b = max(t0b, __float_as_uint(b > 0.0f ? b : 0.0f));
        }
    }
    const SumMaxMin r = block_sum_max_min(negf, t0b, 0u, S.tk.red);  // sum: low half = #negative, high half = #non-finite
    if (tid == 0) {
        S.tk.count = 0;
        S.tk.tau = (r.sum || a.after_score != nullptr) ? 0u : r.mx;  // the bounds speak of the k best of ALL docs, not of those after a row
        S.ub_bits = 0xFFFFFFFFu;
        S.ub_doc = 0;
        if (a.after_score != nullptr) {  // rows come back as GLOBAL ids: the bound is compared in shard-local ids
            const int64_t d = (int64_t)a.after_doc[q] - a.w.doc_base;
            S.ub_bits = __float_as_uint(fmaxf(a.after_score[q], 0.0f));
            S.ub_doc = d < -1 ? -1 : d > 0x7FFFFFFFll ? 0x7FFFFFFF : (int)d;
        }
    }
    hash_mode(S);
    return r.sum >= 0x10000u;
}

// Overflow packer (a unit of several tiles with more than DENSE_MIN postings, on an index whose tiles are too large for the
// wave-level dense path): the unit's tiles [ja, jb) are packed greedily into groups of <= DENSE_MIN postings, each a hash
// unit; a single tile above that is accumulated densely.  Thread i < nt owns term i (base / skip_row).
template <typename VT, bool AFTER, bool CP>
__device__ void packed_unit(ScoreShared &S, const IndexView &ix, int nt, int k, int64_t base, const int32_t *skip_row, int ja, int jb,
                            bool append_scan) {
    const int tid = threadIdx.x;
    const int nt_tiles = jb - ja;
    for (int j = tid; j <= nt_tiles; j += THREADS) S.ptile[j] = 0;
    __syncthreads();
    if (tid < nt) {
        int prev = skip_row[ja];
        for (int j = 0; j < nt_tiles; ++j) {
            const int cur = skip_row[ja + j + 1];
            if (cur != prev) atomicAdd(&S.ptile[j], cur - prev);
            prev = cur;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int ng = 0, acc_p = 0;
        S.grp[0] = 0;
        for (int j = 0; j < nt_tiles; ++j) {
            const int pj = S.ptile[j];
            if (acc_p > 0 && acc_p + pj > DENSE_MIN) {
                S.grp[++ng] = j;
                acc_p = 0;
            }
            acc_p += pj;
        }
        S.grp[++ng] = nt_tiles;
        S.n_grp = ng;
    }
    __syncthreads();
    const int ng = S.n_grp;
    for (int g = 0; g < ng; ++g) {
        const int ga = ja + S.grp[g], gb = ja + S.grp[g + 1];
        int glo = 0, ghi = 0;
        if (tid < nt) {
            glo = skip_row[ga];
            ghi = skip_row[gb];
        }
        const int glen = ghi - glo;
        const unsigned GP = block_sum((unsigned)glen, S.tk.red);
        if (GP == 0) continue;
        set_runs(S, nt, base + glo, glen);
        const unsigned n_old = S.tk.count;  // stable here: nothing appends before the barrier
        __syncthreads();
        if (GP <= (unsigned)DENSE_MIN) {
            hash_unit<VT, AFTER, CP>(S, ix, nt, glen, k, ja << ix.tile_log2);
        } else {  // one dense tile, the group's LAST: a group only closes once it holds postings, so empty tiles may come before it
            const int tile_base = (gb - 1) << ix.tile_log2;
            dense_tile_accumulate<VT, CP>(S, ix, nt, tile_base, true, ja << ix.tile_log2);
            // m_start / m_len are live: the append scan has no overflow area
            if (!(append_scan && dense_tile_append<AFTER>(S, ix, tile_base, k, 1, n_old, 0))) dense_tile_general<AFTER>(S, ix, tile_base, k, 1);
            hash_mode(S);
        }
    }
}

// Queries of more than MAXT terms: tile by tile over [ja, jb), dense accumulators, term passes in ascending order so the
// per-doc summation order is unchanged.
template <typename VT, bool AFTER, bool CP>
__device__ void many_term_tiles(ScoreShared &S, const srx_score_launch &a, int t0, int nt_all, int ja, int jb, bool append_scan) {
    const int tid = threadIdx.x;
    const IndexView &ix = a.w.ix;
    const int row = ix.n_tiles + 1;
    const int n_pass = (nt_all + MAXT - 1) / MAXT;
    for (int j = ja; j < jb; ++j) {
        const int tile_base = j << ix.tile_log2;
        const unsigned n_old = S.tk.count;  // stable: the barrier that opens every pass comes before any append
        for (int pass = 0; pass < n_pass; ++pass) {
            const int nt = min(MAXT, nt_all - pass * MAXT);
            __syncthreads();
            if (tid < nt) {
                const int term = a.w.q_term[t0 + pass * MAXT + tid];
                const int32_t *skip_row = ix.tile_skip + (int64_t)term * row;
                const int lo = skip_row[j], hi = skip_row[j + 1];
                set_runs(S, nt, ix.term_ptr[term] + lo, hi - lo);
                S.m_idf[tid] = ix.idf[term];
                S.m_qw[tid] = a.w.q_weight[t0 + pass * MAXT + tid];
            }
            __syncthreads();
            dense_tile_accumulate<VT, CP>(S, ix, nt, tile_base, pass == 0, ((j / ix.unit_tiles) * ix.unit_tiles) << ix.tile_log2);
        }
        // m_start / m_len are live: the append scan has no overflow area
        if (!(append_scan && dense_tile_append<AFTER>(S, ix, tile_base, a.w.k, 1, n_old, 0))) dense_tile_general<AFTER>(S, ix, tile_base, a.w.k, 1);
    }
}

// Closes a work item: the list shrinks to its k best and goes to the split's candidate list (unordered; the merge kernel
// ranks) -- or, for an unsplit query, straight to the final row.
__device__ void emit_item(ScoreShared &S, const srx_score_launch &a, int q, int nsq, int64_t list) {
    const int tid = threadIdx.x;
    const int k = a.w.k;
    int32_t *__restrict__ cand_doc = a.w.cand_doc, *__restrict__ cand_count = a.w.cand_count;
    float *__restrict__ cand_score = a.w.cand_score;
    __syncthreads();
    topk_shrink(k, S.tk, S.tbl);
    if (nsq == 1 && a.w.out_doc != nullptr) {
        // An unsplit query is ONE work item: this block holds everything tier 1 did not score.  Fold tier 1's list of the
        // same query in (it was complete before this kernel started; its docs come from other units), rank, and write the
        // final row here -- the merge kernel only ever sees split queries.
        const int64_t l1 = (int64_t)q * a.w.lists_per_q;
        const int c1 = min(max(cand_count[l1], 0), k);
        const unsigned tau = S.tk.tau;  // k entries >= tau are in the list once a selection has run: nothing below can enter
        unsigned ub[KPT];
        int ud[KPT];
#pragma unroll
        for (int j = 0; j < KPT; ++j) {
            const int i = tid + j * THREADS;
            const unsigned b = i < c1 ? __float_as_uint(cand_score[l1 * k + i]) : 0u;
            ub[j] = (b >= tau && b != 0u) ? b : 0u;
            ud[j] = i < c1 ? cand_doc[l1 * k + i] : 0;
        }
        __syncthreads();
        topk_fold<KPT, false>(ub, ud, k, S.tk, S.tbl);
        __syncthreads();
        block_rank_emit(S.tk, reinterpret_cast<unsigned long long *>(S.tbl), k, a.w.doc_base, a.w.out_doc + (int64_t)q * a.w.out_row_stride,
                        a.w.out_score + (int64_t)q * a.w.out_row_stride, a.w.out_count + (int64_t)q * a.w.out_cnt_stride);
        if (tid == 0) cand_count[l1] = -1;  // final (as when tier 1 finishes a query on its own)
        return;
    }
    const unsigned cnt = S.tk.count;
    const int64_t o = list * k;
    for (unsigned i = tid; i < cnt; i += THREADS) {
        cand_doc[o + i] = S.tk.doc[i];
        cand_score[o + i] = __uint_as_float(S.tk.bits[i]);
    }
    if (tid == 0) cand_count[list] = (int)cnt;
}

// One work item = one (query, split of the doc range): which of the paths above serves which of its units.
template <typename VT, bool AFTER, bool CP>
__device__ void score_block(ScoreShared &S, int bid, const srx_score_launch &a) {
    const int tid = threadIdx.x;
    const IndexView &ix = a.w.ix;
    const int32_t *__restrict__ q_term = a.w.q_term;
    const float *__restrict__ q_weight = a.w.q_weight;
    const int k = a.w.k, tps = a.tpu, dbg = a.w.dbg;  // tps: tiles per unit
    int q, split, nsq;
    decode_item(bid, a.w.n_whole, a.w.n_splits, q, split, nsq);
    if (q >= a.w.nq) return;
    const int64_t list = (int64_t)q * a.w.lists_per_q + a.w.n_splits + split;  // tier-2 lists follow the tier-1 lists
    const int t0 = a.w.q_ptr[q];
    const int nt_all = a.w.q_ptr[q + 1] - t0;
    // this split's supertiles [su_lo, su_hi)
    const int su_lo = (int)(((int64_t)a.w.n_super * split) / nsq);
    const int su_hi = (int)(((int64_t)a.w.n_super * (split + 1)) / nsq);
    // Tier 2 takes the whole query when tier 1 cannot serve it, otherwise only the units tier 1 flagged.
    const bool all_units = tier1_cannot_serve(ix, nt_all, k, tps, dbg);
    const unsigned *__restrict__ my_ovf = a.w.ovf + (int64_t)bid * a.w.ovf_words;  // the flags tier 1's item of the same (query, split) left
    bool any = all_units && nt_all > 0;
    if (!all_units && nt_all > 0)
        for (int wd = su_lo >> 5; wd <= (su_hi - 1) >> 5 && su_lo < su_hi; ++wd) any = any || (my_ovf[wd] != 0u);
    if (!any) {  // uniform
        if (tid == 0) a.w.cand_count[list] = 0;
        return;
    }
    const bool nonfinite = open_item(S, a, q, t0, nt_all);
    const bool append_scan = !(dbg & SRX_DBG_WAVE_DENSE_GENERAL);  // dense tiles try the append scan before the general selection

    if (nt_all > MAXT) {
        many_term_tiles<VT, AFTER, CP>(S, a, t0, nt_all, su_lo * tps, min(su_hi * tps, ix.n_tiles), append_scan);
        emit_item(S, a, q, nsq, list);
        return;
    }
    // ---- thread i owns term i ----
    const int nt = nt_all;
    const int row = ix.n_tiles + 1;
    int64_t base = 0;
    const int32_t *skip_row = ix.tile_skip;
    if (tid < nt) {
        const int term = q_term[t0 + tid];
        base = ix.term_ptr[term];
        skip_row = ix.tile_skip + (int64_t)term * row;
        S.m_idf[tid] = ix.idf[term];
        S.m_qw[tid] = q_weight[t0 + tid];
    }
    // wave-level dense path (tiles of <= 4096 docs, <= 64 terms): lane i of EVERY wave carries term i
    const bool wave_dense = (4 << ix.tile_log2) <= TBL_WORDS && nt <= 64 && !(dbg & SRX_DBG_NO_WAVE_DENSE);
    int64_t wbase = 0;
    const int32_t *wskip = ix.tile_skip;
    float w_idf = 0.f, w_qw = 0.f;
    if (wave_dense && (tid & 63) < nt) {
        const int term = q_term[t0 + (tid & 63)];
        wbase = ix.term_ptr[term];
        wskip = ix.tile_skip + (int64_t)term * row;
        w_idf = ix.idf[term];
        w_qw = q_weight[t0 + (tid & 63)];
    }
    // one-tile units + finite weights: the unmasked form (see wave_dense_accumulate)
    const bool wd_aligned = ix.unit_tiles == 1 && !nonfinite && !(dbg & SRX_DBG_WAVE_DENSE_MASKED);
    auto dense_quads = [&](int ja, int jb) {  // tiles [ja, jb): four at a time, one per wave, no block barriers inside
        // my term's run boundaries of the NEXT group's tile are loaded while this group is accumulated (a dependent
        // load at the top of every group exposed one memory round trip per four tiles); clamped index, no branch
        const int jlast = ix.n_tiles - 1;
        int a_n = gload_i32(wskip + min(ja + (tid >> 6), jlast)), b_n = gload_i32(wskip + min(ja + (tid >> 6), jlast) + 1);
        for (int j0 = ja; j0 < jb; j0 += WAVES) {
            const int j = j0 + (tid >> 6);
            const bool has_tile = j < jb;
            const bool mine = has_tile && (tid & 63) < nt;
            const int lo = mine ? a_n : 0, hi = mine ? b_n : 0;
            a_n = gload_i32(wskip + min(j + WAVES, jlast));
            b_n = gload_i32(wskip + min(j + WAVES, jlast) + 1);
            if (wd_aligned)
                wave_dense_accumulate<VT, true, CP>(S, ix, nt, (int64_t)j << ix.tile_log2, has_tile, wbase + lo, hi - lo, w_idf, w_qw);
            else
                wave_dense_accumulate<VT, false, CP>(S, ix, nt, (int64_t)j << ix.tile_log2, has_tile, wbase + lo, hi - lo, w_idf, w_qw);
            const unsigned n_old = S.tk.count;  // stable here: nothing appends before the barrier
            __syncthreads();
            // m_start / m_len are idle on this path: the append scan has the whole overflow area
            if (!(append_scan && dense_tile_append<AFTER>(S, ix, j0 << ix.tile_log2, k, WAVES, n_old, OVF_CAP)))
                dense_tile_general<AFTER>(S, ix, j0 << ix.tile_log2, k, WAVES);
        }
        if (S.tk.count > (unsigned)KMAX) list_compact_select(S, k, S.tk.count);  // uniform (stable since the last barrier): the overflow area goes back to its owners
        hash_mode(S);
    };
    if (all_units && wave_dense) {
        // tier 2 has the whole query (k or the term count rules tier 1 out): units mean nothing here, the split's tile
        // range goes through the wave-level dense path in full groups of four tiles
        dense_quads(su_lo * tps, min(su_hi * tps, ix.n_tiles));
    } else
    for (int su = su_lo; su < su_hi; ++su) {
        if (!all_units && !((my_ovf[su >> 5] >> (su & 31)) & 1u)) continue;  // uniform
        const int ja = su * tps, jb = min(ja + tps, ix.n_tiles);  // the unit's tiles
        int lo = 0, hi = 0;
        if (tid < nt) {
            lo = gload_i32(skip_row + min(ja, ix.n_tiles));
            hi = gload_i32(skip_row + min(ja + tps, ix.n_tiles));
        }
        const int my_len = hi - lo;
        const unsigned P = block_sum((unsigned)my_len, S.tk.red);
        if (P == 0) continue;  // uniform
        // many-term queries on a one-tile unit: all terms at once (flat_tile) instead of term by term
        const bool flat_ok = tps == 1 && nt >= FLAT_MIN_TERMS && P <= (unsigned)FLAT_CAP && !(dbg & SRX_DBG_NO_FLAT_TILES);
        bool served = false;
        if (flat_ok) {
            set_runs(S, nt, base + lo, my_len);
            __syncthreads();
            served = flat_tile<VT, AFTER, CP>(S, ix, nt, my_len, su << ix.tile_log2, k);
            hash_mode(S);
        }
        if (served) continue;
        if (P <= (unsigned)DENSE_MIN) {
            set_runs(S, nt, base + lo, my_len);
            __syncthreads();
            hash_unit<VT, AFTER, CP>(S, ix, nt, my_len, k, ja << ix.tile_log2);
        } else if (wave_dense) {
            dense_quads(ja, jb);
        } else {
            packed_unit<VT, AFTER, CP>(S, ix, nt, k, base, skip_row, ja, jb, append_scan);
        }
    }
    emit_item(S, a, q, nsq, list);
}

// Tier-2 kernel: a fixed grid of workgroups drains the worklist of (query, split) blocks that tier 1 could not
// finish (flagged units, > 64 terms, k > 112).  work[0] = number of entries, work[1..] = block ids.
template <typename VT, bool AFTER, bool CP>
__global__ __launch_bounds__(THREADS, 2) void srx_score_kernel(const srx_score_launch a) {
    __shared__ ScoreShared S;
    static_assert(2 * sizeof(ScoreShared) <= 160 * 1024, "the launch bounds: two workgroups share a CU's 160 KiB of LDS");
    const int *__restrict__ work = a.w.work;
    const int n_work = work[0];
    if (a.hint != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *a.hint = n_work;
    for (int w = blockIdx.x; w < n_work; w += gridDim.x) {
        __syncthreads();  // the previous block's LDS state is dead
        score_block<VT, AFTER, CP>(S, work[1 + w], a);
    }
}

template <typename VT, bool AFTER, bool CP>
void launch_instance(const srx_score_launch &a, unsigned grid, hipStream_t stream) {
    hipLaunchKernelGGL((srx_score_kernel<VT, AFTER, CP>), dim3(grid), dim3(THREADS), 0, stream, a);
}
template <typename VT, bool AFTER>
void launch_copy(const srx_score_launch &a, unsigned grid, hipStream_t stream) {  // no canonical blocks: tier 2 reads the compact copy too
    a.w.ix.post == nullptr ? launch_instance<VT, AFTER, true>(a, grid, stream) : launch_instance<VT, AFTER, false>(a, grid, stream);
}
template <typename VT>
void launch_after(const srx_score_launch &a, unsigned grid, hipStream_t stream) {  // srx_search_after: every candidate is tested against the bound
    a.after_score != nullptr ? launch_copy<VT, true>(a, grid, stream) : launch_copy<VT, false>(a, grid, stream);
}

}  // namespace

// The launcher names the three choices once each -- value type, search-after, compact copy -- and with them the eight
// instances in a fixed order (float before __half, AFTER before plain, CP before canonical): the order the instances are
// first named in decides which helpers the compiler inlines, so it is part of the generated code.
int srx_launch_score_kernel(const srx_score_launch &a, int val_type, unsigned grid, hipStream_t stream) {
    val_type == SRX_VAL_F32 ? launch_after<float>(a, grid, stream) : launch_after<__half>(a, grid, stream);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
