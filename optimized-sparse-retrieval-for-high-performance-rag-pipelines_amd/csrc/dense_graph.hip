// dense_graph.hip -- the graph dense index (include/graph/sparse_rx_graph.h): a fixed-degree neighbour graph over the half
// index's rows, walked by a beam search, and the two integer kernels that build the graph from k-nearest lists.  Replaces
// nothing in the reference project: it has no approximate index.
//
//   search    one workgroup (four waves) per query, one launch, no workspace.  LDS holds the whole state of a walk:
//               qfrag    the query rounded once, as the A pieces of every k-step (2 pieces of 16 bytes per k-step, <= 2 KiB);
//               visited  an open-addressing table of row numbers (dynamic, a power of two >= twice the call's visit budget,
//                        <= 16 384 slots = 64 KiB); an LDS compare-and-swap inserts, so of several lanes that hold one id
//                        exactly one wins; probe loops are bounded by the slot count;
//               beam     <= 512 sorted 64-bit keys, and as many keys of the step's new docs: a key is the order-mapped value,
//                        the inverted row and the expanded bit, so "larger key" is (value descending, doc ascending);
//               cand     the step's surviving neighbours, ballot-compacted.
//             A step: wave 0 takes the first <= p unexpanded keys of the beam; every thread reads <= 2 entries of the parents'
//             graph rows and offers them to the table; the survivors are scored in tiles of 32, the waves taking alternate
//             tiles, each lane gathering its row's pieces straight from the fragment layout (hf_piece) four k-steps ahead and
//             the next tile's first pieces before the last MFMAs of this one -- the whole k range is one chain, no split-K, so
//             the bits are those of srx_dense_score_docs_half; the new keys are sorted by a bitonic network (stages that stay
//             inside a wave's 128 keys need no workgroup barrier), one max pass against the reversed beam keeps the best, and a
//             bitonic merge orders them: the 1 024 keys are never sorted as a whole.
//   prune     one workgroup per node: the node's own row goes into a small LDS table (id -> first position), the rows of its
//             neighbours are read as coalesced row loads, one lookup per element; detour counts are LDS integers.
//   merge     one wave per node: the interleaved sequence in LDS, a quadratic duplicate test over <= 96 entries, a ballot
//             compaction in order.
// No scratch, no atomics on global memory, nothing waits for another workgroup.
#include "half_common.h"
#include "graph/sparse_rx_graph.h"

namespace {

constexpr int GS_MAX_L = 512;         // beam width
constexpr int GS_MAX_NEW = 512;       // docs one step (or the seeds) can add: width * degree, n_seed
constexpr int GS_MAX_WIDTH = 8;
constexpr int GS_MAX_ITER = 1024;
constexpr int GS_MAX_BUDGET = 8192;   // n_seed + max_iter * width * degree
constexpr int GS_MIN_SLOT_LOG2 = 6;
static_assert(THREADS == 256 && WAVES == 4, "the sort gives wave w the keys 128 w .. 128 w + 127; two beam entries per thread");
static_assert(2 * GS_MAX_BUDGET <= 16384, "the visited table is at most 16 384 slots (64 KiB)");

struct GraphSearchArgs {
    const hf_v4i *corpus;
    const int32_t *graph;
    const float *queries;
    const int32_t *seed_doc;      // null: spread rows
    const uint32_t *filter_bits;  // null: no filter
    const int32_t *q_filter;
    int64_t filter_words;
    int32_t *out_doc;
    float *out_score;
    int32_t *out_count, *out_stat;
    int64_t n_docs, doc_base;
    int ks, deg_log2, L, width, max_iter, n_seed, k, slot_log2;
    float score_offset;
};

// (value descending, row ascending) as one unsigned order; bit 0: expanded.  Never 0: row <= 2^31 - 3.
__device__ __forceinline__ unsigned long long gs_key(float v, int row) {
    const unsigned b = __float_as_uint(v);
    const unsigned o = (b & 0x80000000u) != 0u ? ~b : (b | 0x80000000u);
    return ((unsigned long long)o << 32) | ((unsigned long long)(0x7FFFFFFFu - (unsigned)row) << 1);
}
__device__ __forceinline__ int gs_key_row(unsigned long long key) { return (int)(0x7FFFFFFFu - ((unsigned)key >> 1)); }
__device__ __forceinline__ float gs_key_value(unsigned long long key) {
    const unsigned o = (unsigned)(key >> 32);
    return __uint_as_float((o & 0x80000000u) != 0u ? (o & 0x7FFFFFFFu) : ~o);
}

// true: `row` was not in the table and now is (this lane won the slot)
__device__ __forceinline__ bool gs_visit(int *tbl, int slot_log2, int row) {
    const unsigned mask = (1u << slot_log2) - 1u;
    unsigned h = ((unsigned)row * 2654435761u) >> (32 - slot_log2);
    for (unsigned n = 0; n <= mask; ++n) {  // the table holds at most half its slots: an empty one is met long before
        const int old = atomicCAS(&tbl[h], -1, row);
        if (old == -1) return true;
        if (old == row) return false;
        h = (h + 1u) & mask;
    }
    return false;
}
// the wave's fresh rows appended to cand (any order: the keys are sorted afterwards)
__device__ __forceinline__ void gs_push(bool fresh, int row, int *cand, int *n_new) {
    const unsigned long long m = __ballot(fresh);
    if (m == 0ull) return;  // uniform
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
    int base = 0;
    if (lane == leader) base = atomicAdd(n_new, __popcll(m));
    base = __shfl(base, leader);
    if (fresh) cand[base + (int)lane_rank(m)] = row;
}
// what orders two stages of a bitonic network: a stage whose partners are <= 64 apart stays inside the 128 keys of one wave
__device__ __forceinline__ void gs_stage_sync(int j) {
    if (j > 64)
        __syncthreads();
    else
        wsync();
}

template <int TYPE>
__global__ __launch_bounds__(THREADS) void srx_graph_search_kernel(GraphSearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char gs_lds[];
    int *tbl = reinterpret_cast<int *>(gs_lds);
    __shared__ unsigned long long beam[GS_MAX_L], fresh[GS_MAX_NEW];
    __shared__ hf_v4i qfrag[128];  // [k-step][half]
    __shared__ int cand[GS_MAX_NEW];
    __shared__ int parent[GS_MAX_WIDTH];
    __shared__ int n_new, n_par, wcnt[2][WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int64_t q = blockIdx.x;
    const int ks = a.ks, L = a.L;
    int Lp = 32;  // the beam's power of two
    while (Lp < L) Lp <<= 1;

    for (int i = tid; i < (1 << a.slot_log2); i += THREADS) tbl[i] = -1;
    for (int i = tid; i < GS_MAX_L; i += THREADS) beam[i] = 0ull;
    if (tid < 2 * ks) {
        const hf_v4f *src = reinterpret_cast<const hf_v4f *>(a.queries + q * (ks * 16) + 16 * (tid >> 1) + 8 * (tid & 1));
        qfrag[tid] = hf_round8<TYPE>(src[0], src[1]);
    }
    if (tid == 0) n_new = 0;
    __syncthreads();

    int steps = 0, scored = 0;
    for (int it = 0; it <= a.max_iter; ++it) {
        // ---- the candidates of this round: the seeds, then the neighbours of the step's parents ----
        int total;
        if (it == 0) {
            total = a.n_seed;
        } else {
            if (wave == 0) {
                int found = 0;
                for (int c0 = 0; c0 < L && found < a.width; c0 += 64) {
                    const int i = c0 + lane;
                    const unsigned long long key = i < L ? beam[i] : 0ull;
                    const bool open = key != 0ull && (key & 1ull) == 0ull;
                    const unsigned long long m = __ballot(open);
                    const int rank = found + (int)lane_rank(m);
                    if (open && rank < a.width) {
                        parent[rank] = gs_key_row(key);
                        beam[i] = key | 1ull;
                    }
                    found += __popcll(m);
                }
                if (lane == 0) n_par = found < a.width ? found : a.width;
            }
            __syncthreads();
            if (n_par == 0) break;  // uniform
            ++steps;
            total = n_par << a.deg_log2;
        }
        for (int i = tid; i < GS_MAX_NEW; i += THREADS) fresh[i] = 0ull;
        for (int i0 = 0; i0 < total; i0 += THREADS) {
            const int i = i0 + tid;
            int row = -1;
            if (i < total) {
                int64_t local;
                if (it > 0)
                    local = gload_i32(a.graph + (((int64_t)parent[i >> a.deg_log2]) << a.deg_log2) + (i & ((1 << a.deg_log2) - 1)));
                else if (a.seed_doc != nullptr)
                    local = (int64_t)gload_i32(a.seed_doc + q * a.n_seed + i) - a.doc_base;
                else
                    local = (int64_t)i * a.n_docs / a.n_seed;
                if (local >= 0 && local < a.n_docs) row = (int)local;
            }
            const bool won = row >= 0 && gs_visit(tbl, a.slot_log2, row);
            gs_push(won, row, cand, &n_new);
        }
        __syncthreads();
        const int nn = n_new;  // uniform
        scored += nn;
        if (nn > 0) {
            // ---- score: tiles of 32 rows, the waves take alternate tiles, one chain per row ----
            const int n_tiles = (nn + 31) >> 5;
            auto tile_row = [&](int t) __attribute__((always_inline)) { return t * 32 + r < nn ? cand[t * 32 + r] : -1; };
            auto load4 = [&](hf_v4i(&B)[4], int row, int s0) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    B[u] = (hf_v4i){0, 0, 0, 0};
                    if (row >= 0) B[u] = a.corpus[hf_piece(row, ks, s0 + u, h)];
                }
            };
            int t = wave, row = -1;
            hf_v4i B[4];
            if (t < n_tiles) {
                row = tile_row(t);
                load4(B, row, 0);
            }
            while (t < n_tiles) {
                const int tn = t + WAVES;
                const int rown = tn < n_tiles ? tile_row(tn) : -1;
                hf_v16f acc;
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
                for (int s0 = 0; s0 < ks; s0 += 4) {  // ks is a multiple of 4; ascending k from +0.0f
                    hf_v4i Bn[4], A[4];
                    if (s0 + 4 < ks)
                        load4(Bn, row, s0 + 4);
                    else
                        load4(Bn, rown, 0);  // the next tile's first pieces, in flight over these MFMAs (zeros: no next tile)
#pragma unroll
                    for (int u = 0; u < 4; ++u) A[u] = qfrag[2 * (s0 + u) + h];
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc = hf_mfma<TYPE>(A[u], B[u], acc);
#pragma unroll
                    for (int u = 0; u < 4; ++u) B[u] = Bn[u];
                }
                if (h == 0 && row >= 0) {  // lanes 0 .. 31, register 0: row 0 of the tile, column = candidate r
                    float v = acc[0] + a.score_offset;
                    v = v == 0.0f ? 0.0f : v;  // one zero
                    fresh[t * 32 + r] = gs_key(v, row);
                }
                t = tn;
                row = rown;
            }
        }
        __syncthreads();
        if (tid == 0) n_new = 0;  // every thread has read it; the next append is barriers away
        if (nn > 0) {
            // ---- sort the new keys, descending ----
            int M = 1;
            while (M < nn) M <<= 1;
            for (int kk = 2; kk <= M; kk <<= 1)
                for (int j = kk >> 1; j > 0; j >>= 1) {
                    if (j > 64) __syncthreads();  // the stage before may have been a wave's own
                    if (tid < (M >> 1)) {
                        const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), l = i | j;
                        const unsigned long long x = fresh[i], y = fresh[l];
                        if ((x < y) == ((i & kk) == 0)) {
                            fresh[i] = y;
                            fresh[l] = x;
                        }
                    }
                    gs_stage_sync(j);
                }
            // ---- the best P of (beam, new): one max pass against the reversed new keys leaves a bitonic sequence ----
            const int P = Lp > M ? Lp : M;
            __syncthreads();
            for (int i = tid; i < P; i += THREADS) {
                const unsigned long long y = fresh[P - 1 - i];
                if (y > beam[i]) beam[i] = y;
            }
            __syncthreads();
            for (int j = P >> 1; j > 0; j >>= 1) {
                if (tid < (P >> 1)) {
                    const int i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), l = i | j;
                    const unsigned long long x = beam[i], y = beam[l];
                    if (x < y) {
                        beam[i] = y;
                        beam[l] = x;
                    }
                }
                gs_stage_sync(j);
            }
            __syncthreads();
            for (int i = L + tid; i < P; i += THREADS) beam[i] = 0ull;  // the beam is L wide
            __syncthreads();
        }
    }

    // ---- result: the beam in order, allowed and > 0, the first k ----
    const uint32_t *frow = nullptr;
    if (a.filter_bits != nullptr) {
        const int fr = a.q_filter != nullptr ? gload_i32(a.q_filter + q) : 0;
        if (fr >= 0) frow = a.filter_bits + (int64_t)fr * a.filter_words;
    }
    unsigned long long key2[2], m2[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int i = p * THREADS + tid;
        key2[p] = i < L ? beam[i] : 0ull;
        bool keep = key2[p] != 0ull && gs_key_value(key2[p]) > 0.0f;
        if (keep && frow != nullptr) {
            const int row = gs_key_row(key2[p]);
            keep = ((frow[row >> 5] >> (row & 31)) & 1u) != 0u;
        }
        m2[p] = __ballot(keep);
        if (lane == 0) wcnt[p][wave] = __popcll(m2[p]);
    }
    __syncthreads();
    int before[2] = {0, 0}, all = 0;
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int w = 0; w < WAVES; ++w) {
            const int c = wcnt[p][w];
            if (p == 0 && w < wave) before[0] += c;
            if (p == 0 || w < wave) before[1] += c;
            all += c;
        }
    int32_t *od = a.out_doc + q * a.k;
    float *os = a.out_score + q * a.k;
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int pos = before[p] + (int)lane_rank(m2[p]);
        if (((m2[p] >> lane) & 1ull) != 0ull && pos < a.k) {
            od[pos] = (int32_t)(a.doc_base + gs_key_row(key2[p]));
            os[pos] = gs_key_value(key2[p]);
        }
    }
    const int count = all < a.k ? all : a.k;
    for (int i = count + tid; i < a.k; i += THREADS) {
        od[i] = -1;
        os[i] = 0.0f;
    }
    if (tid == 0) {
        a.out_count[q] = count;
        if (a.out_stat != nullptr) {
            a.out_stat[2 * q] = steps;
            a.out_stat[2 * q + 1] = scored;
        }
    }
}

// ================================================================================================ prune
constexpr int GP_MAX_D0 = 128;
constexpr int GP_SLOTS = 512;  // >= 4 x the entries of a row
__device__ __forceinline__ unsigned gp_hash(int id) { return ((unsigned)id * 2654435761u) >> 23; }
// the first valid position of id `z` in the node's own row, -1: not there
__device__ __forceinline__ int gp_lookup(const int *key, const int *pos, int z, int64_t n, int64_t x) {
    if (z < 0 || z >= n || z == x) return -1;
    unsigned hh = gp_hash(z);
    for (int t = 0; t < GP_SLOTS; ++t) {
        const int kk = key[hh];
        if (kk == z) return pos[hh];
        if (kk == -1) return -1;
        hh = (hh + 1u) & (GP_SLOTS - 1);
    }
    return -1;
}

__global__ __launch_bounds__(THREADS) void srx_graph_prune_kernel(const int32_t *__restrict__ knn, int64_t n, int d0, int degree,
                                                                   int32_t *__restrict__ out) {
    __shared__ int key[GP_SLOTS], pos[GP_SLOTS], own[GP_MAX_D0], valid[GP_MAX_D0], det[GP_MAX_D0], mark[WAVES][GP_MAX_D0];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t x = blockIdx.x;
    for (int i = tid; i < GP_SLOTS; i += THREADS) {
        key[i] = -1;
        pos[i] = 0x7FFFFFFF;
        (&mark[0][0])[i] = 0;
    }
    if (tid < GP_MAX_D0) det[tid] = 0;
    __syncthreads();
    if (tid < d0) {
        const int y = gload_i32(knn + x * d0 + tid);
        own[tid] = y;
        if (y >= 0 && y < n && y != x) {
            unsigned hh = gp_hash(y);
            for (int t = 0; t < GP_SLOTS; ++t) {  // <= 128 entries in 512 slots
                const int old = atomicCAS(&key[hh], -1, y);
                if (old == -1 || old == y) {
                    atomicMin(&pos[hh], tid);
                    break;
                }
                hh = (hh + 1u) & (GP_SLOTS - 1);
            }
        }
    }
    __syncthreads();
    if (tid < d0) valid[tid] = gp_lookup(key, pos, own[tid], n, x) == tid ? 1 : 0;
    __syncthreads();
    for (int i = wave; i < d0; i += WAVES) {  // one neighbour's row per wave and trip
        if (valid[i] == 0) continue;           // uniform
        const int32_t *yrow = knn + (int64_t)own[i] * d0;
        for (int rr = lane; rr < d0; rr += 64) {
            const int j = gp_lookup(key, pos, gload_i32(yrow + rr), n, x);
            if (j > i && rr < j && atomicExch(&mark[wave][j], i + 1) != i + 1) atomicAdd(&det[j], 1);  // each i once per j
        }
    }
    __syncthreads();
    if (tid < d0 && valid[tid] != 0) {
        const int mine = det[tid];
        int rank = 0;
        for (int j = 0; j < d0; ++j) rank += (valid[j] != 0 && (det[j] < mine || (det[j] == mine && j < tid))) ? 1 : 0;
        if (rank < degree) out[x * degree + rank] = own[tid];
    }
    if (tid < degree) {
        int nv = 0;
        for (int j = 0; j < d0; ++j) nv += valid[j];
        if (tid >= nv) out[x * degree + tid] = -1;
    }
}

// ================================================================================================ merge
constexpr int GM_MAX_SEQ = 96;  // degree + degree / 2
__global__ __launch_bounds__(THREADS) void srx_graph_merge_kernel(const int32_t *__restrict__ fwd, int64_t n, int degree,
                                                                   const int64_t *__restrict__ rev_ptr, const int32_t *__restrict__ rev_src,
                                                                   int32_t *__restrict__ out) {
    __shared__ int seq[WAVES][GM_MAX_SEQ];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t y = (int64_t)blockIdx.x * WAVES + wave;
    if (y >= n) return;  // whole waves leave; no workgroup barrier below
    const int half = degree >> 1, len = degree + half;
    const int64_t rs = rev_ptr[y], span = rev_ptr[y + 1] - rs;
    const int rc = (int)(span < 0 ? 0 : span > half ? half : span);
    for (int e = lane; e < len; e += 64) {
        int id = -1;
        if (e < half)
            id = gload_i32(fwd + y * degree + e);
        else if (e < 2 * half) {
            if (e - half < rc) id = gload_i32(rev_src + rs + (e - half));
        } else
            id = gload_i32(fwd + y * degree + (e - half));
        seq[wave][e] = (id >= 0 && id < n && id != y) ? id : -1;
    }
    wsync();
    unsigned long long m[2];
    int ids[2];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int e = p * 64 + lane;
        ids[p] = e < len ? seq[wave][e] : -1;
        bool keep = ids[p] >= 0;
        for (int e2 = 0; e2 < e && keep; ++e2) keep = seq[wave][e2] != ids[p];
        m[p] = __ballot(keep);
    }
    const int first = __popcll(m[0]), total = first + __popcll(m[1]);
#pragma unroll
    for (int p = 0; p < 2; ++p) {
        const int at = (p == 0 ? 0 : first) + (int)lane_rank(m[p]);
        if (((m[p] >> lane) & 1ull) != 0ull && at < degree) out[y * degree + at] = ids[p];
    }
    for (int t = total + lane; t < degree; t += 64) out[y * degree + t] = -1;
}

// ================================================================================================ host side
bool type_ok(int32_t type) { return type == SRX_HALF_F16 || type == SRX_HALF_BF16; }
bool degree_ok(int32_t degree) { return degree == 16 || degree == 32 || degree == 64; }

// prune and merge: 1 = nothing to do, 0 = go on, < 0 = refused
int build_check(const char *who, int64_t n, int32_t degree) {
    if (n < 0 || n > SRX_FILTER_MAX_DOCS) return fail(SRX_ERR_INVALID, "%s: n out of range", who);
    if (!degree_ok(degree)) return fail(SRX_ERR_INVALID, "%s: degree must be 16, 32 or 64", who);
    return n == 0 ? 1 : 0;
}

}  // namespace

SRX_API int srx_graph_search(const srx_graph_desc *d, const float *queries, int32_t nq, int32_t itopk, int32_t width, int32_t max_iter,
                             const int32_t *seed_doc, int32_t n_seed, int32_t k, const srx_doc_filter *filter, int32_t *out_doc,
                             float *out_score, int32_t *out_count, int32_t *out_stat, void *stream_v, float score_offset) {
    const char *who = "srx_graph_search";
    if (d == nullptr) return fail(SRX_ERR_INVALID, "%s: null desc", who);
    if (!type_ok(d->type)) return fail(SRX_ERR_INVALID, "%s: type must be SRX_HALF_F16 or SRX_HALF_BF16", who);
    if (!hf_dim_ok(d->dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 64, <= 1024 (pad the rows with zeros)", who);
    if (!degree_ok(d->degree)) return fail(SRX_ERR_INVALID, "%s: degree must be 16, 32 or 64", who);
    if (d->n_docs < 1 || d->n_docs > SRX_FILTER_MAX_DOCS) return fail(SRX_ERR_INVALID, "%s: n_docs out of range", who);
    if (d->doc_base < 0 || d->doc_base + d->n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: doc_base + n_docs must fit int32", who);
    if (filter != nullptr) {
        const int rc = srx_check_filter(who, filter);
        if (rc != SRX_OK) return rc;
    }
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if (itopk < 32 || itopk > GS_MAX_L || itopk % 32 != 0) return fail(SRX_ERR_INVALID, "%s: itopk must be a multiple of 32 in [32, 512]", who);
    if (width < 1 || width > GS_MAX_WIDTH || width * d->degree > GS_MAX_NEW) return fail(SRX_ERR_INVALID, "%s: need 1 <= width <= 8 and width * degree <= 512", who);
    if (max_iter < 1 || max_iter > GS_MAX_ITER) return fail(SRX_ERR_INVALID, "%s: need 1 <= max_iter <= 1024", who);
    if (n_seed < 1 || n_seed > GS_MAX_NEW) return fail(SRX_ERR_INVALID, "%s: need 1 <= n_seed <= 512", who);
    if (k < 1 || k > itopk) return fail(SRX_ERR_INVALID, "%s: need 1 <= k <= itopk", who);
    const int64_t budget = (int64_t)n_seed + (int64_t)max_iter * width * d->degree;
    if (budget > GS_MAX_BUDGET) return fail(SRX_ERR_INVALID, "%s: the visit budget n_seed + max_iter * width * degree must be <= 8192", who);
    if (nq == 0) return SRX_OK;
    if (!d->corpus || !d->graph) return fail(SRX_ERR_INVALID, "%s: desc holds a null pointer", who);
    if (!queries) return fail(SRX_ERR_INVALID, "%s: null queries", who);
    if (!out_doc || !out_score || !out_count) return fail(SRX_ERR_INVALID, "%s: null output", who);
    if ((uintptr_t)d->corpus & 15) return fail(SRX_ERR_INVALID, "%s: corpus must be 16-byte aligned", who);
    if ((uintptr_t)queries & 15) return fail(SRX_ERR_INVALID, "%s: queries must be 16-byte aligned", who);
    if (((uintptr_t)d->graph | (uintptr_t)seed_doc) & 3) return fail(SRX_ERR_INVALID, "%s: graph / seed_doc must be 4-byte aligned", who);
    GraphSearchArgs a;
    a.corpus = (const hf_v4i *)d->corpus;
    a.graph = d->graph;
    a.queries = queries;
    a.seed_doc = seed_doc;
    a.filter_bits = filter ? filter->bits : nullptr;
    a.q_filter = filter ? filter->q_filter : nullptr;
    a.filter_words = srx_filter_row_words(d->n_docs);
    a.out_doc = out_doc;
    a.out_score = out_score;
    a.out_count = out_count;
    a.out_stat = out_stat;
    a.n_docs = d->n_docs;
    a.doc_base = d->doc_base;
    a.ks = d->dim_pad / 16;
    a.deg_log2 = d->degree == 16 ? 4 : d->degree == 32 ? 5 : 6;
    a.L = itopk;
    a.width = width;
    a.max_iter = max_iter;
    a.n_seed = n_seed;
    a.k = k;
    a.slot_log2 = GS_MIN_SLOT_LOG2;
    while ((1ll << a.slot_log2) < 2 * budget) ++a.slot_log2;  // <= 14
    a.score_offset = score_offset;
    HIP_TRY(hipSetDevice(d->device));
    const size_t dyn = (size_t)4 << a.slot_log2;
    const bool f16 = d->type == SRX_HALF_F16;
    if (dyn > 32768) {  // static + dynamic LDS beyond 64 KiB: opt in (gfx950 has 160 KiB per workgroup)
        if (f16)
            HIP_TRY(hipFuncSetAttribute((const void *)srx_graph_search_kernel<SRX_HALF_F16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
        else
            HIP_TRY(hipFuncSetAttribute((const void *)srx_graph_search_kernel<SRX_HALF_BF16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn));
    }
    if (f16)
        hipLaunchKernelGGL(srx_graph_search_kernel<SRX_HALF_F16>, dim3((unsigned)nq), dim3(THREADS), dyn, (hipStream_t)stream_v, a);
    else
        hipLaunchKernelGGL(srx_graph_search_kernel<SRX_HALF_BF16>, dim3((unsigned)nq), dim3(THREADS), dyn, (hipStream_t)stream_v, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int srx_graph_prune(int32_t device, const int32_t *knn, int64_t n, int32_t d0, int32_t degree, int32_t *out, void *stream_v) {
    const char *who = "srx_graph_prune";
    const int rc = build_check(who, n, degree);
    if (rc < 0) return rc;
    if (d0 < degree || d0 > GP_MAX_D0) return fail(SRX_ERR_INVALID, "%s: need degree <= d0 <= 128", who);
    if (rc == 1) return SRX_OK;
    if (!knn || !out) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)knn | (uintptr_t)out) & 3) return fail(SRX_ERR_INVALID, "%s: knn / out must be 4-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(srx_graph_prune_kernel, dim3((unsigned)n), dim3(THREADS), 0, (hipStream_t)stream_v, knn, n, (int)d0, (int)degree, out);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int srx_graph_merge(int32_t device, const int32_t *fwd, int64_t n, int32_t degree, const int64_t *rev_ptr, const int32_t *rev_src,
                            int32_t *out, void *stream_v) {
    const char *who = "srx_graph_merge";
    const int rc = build_check(who, n, degree);
    if (rc < 0) return rc;
    if (rc == 1) return SRX_OK;
    if (!fwd || !rev_ptr || !rev_src || !out) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if ((((uintptr_t)fwd | (uintptr_t)rev_src | (uintptr_t)out) & 3) || ((uintptr_t)rev_ptr & 7))
        return fail(SRX_ERR_INVALID, "%s: fwd / rev_src / out must be 4-byte aligned, rev_ptr 8-byte", who);
    HIP_TRY(hipSetDevice(device));
    hipLaunchKernelGGL(srx_graph_merge_kernel, dim3((unsigned)((n + WAVES - 1) / WAVES)), dim3(THREADS), 0, (hipStream_t)stream_v, fwd, n, (int)degree,
                       rev_ptr, rev_src, out);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
