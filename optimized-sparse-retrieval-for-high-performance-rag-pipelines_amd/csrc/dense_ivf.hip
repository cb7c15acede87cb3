// dense_ivf.hip -- the IVF dense index (include/ivf/sparse_rx_ivf.h): k-means lists over the half index's rows.  Replaces
// nothing in the reference project: it has no clustered index.  A translation unit of its own, as dense_half.hip is.
//
//   walk      the one GEMM shape of this unit.  A workgroup holds 32 rows of the f32 side (corpus rows to assign, queries to
//             probe with, the queries of a group) as the A operand: rounded once, in fragment order in LDS, dim_pad * 64 bytes
//             (dynamic, at most 64 KiB), a wave's ds_read_b128 of a k-step a contiguous KiB.  The four waves take alternate
//             32-row tiles of B (centroids, a list's rows) straight from memory into registers: a tile is used by one wave
//             only, so staging it through LDS would buy nothing; the next four k-steps' loads are in flight over the MFMAs of
//             these four.  Every output element is ONE chain over s = 0, 1, ... from +0.0f (the half index's), handed to an
//             epilogue with the tile number: D[row = A row][col = B row], lane l holds column l & 31, rows
//             (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
//   assign    epilogue = a running (score, list) per register; 5 shuffles per register, then the waves meet in LDS.
//   probe     epilogue = the score row of the pass; one workgroup per query selects (an 8-bit radix select of its own on
//             order-preserving 32-bit keys: negative scores rank too) and ranks by counting.
//   update    one workgroup per (list, 64 columns): lanes own columns, waves take chunks of 256 members, partials meet in LDS
//             and are added in chunk order.
//   search    clean the probe rows and count per list -> offsets (one workgroup) -> scatter the pairs by list -> scan (list,
//             group of 32 queries) work items, found by a binary search of the group offsets -> rank each pair's strip ->
//             srx_merge_impl.
#include "half_common.h"
#include "ivf_probe.h"
#include "ivf/sparse_rx_ivf.h"

namespace {

constexpr int IVF_MAX_LIST = 65536, IVF_MAX_PROBE = 1024, IVF_PASS = 1024;
constexpr int IVF_CHUNK = 256;  // members per chunk of the update's sums
static_assert(THREADS == 256, "the probe's radix select gives every thread one of its 256 bins");
constexpr int IVF_NPT = 4;      // columns per thread and step of the rank kernel

// ================================================================================================ the A operand
// row i of the block: src(i) = its f32 row or nullptr (zeros); columns at or past dim are zeros.  Consecutive threads read
// consecutive 32-byte pieces of one row.
template <int TYPE, bool VEC, typename Src>
__device__ __forceinline__ void ivf_load_a(hf_v4i *A, int ks, int dim, Src src) {
    const int per_row = 2 * ks;
    for (int i = threadIdx.x; i < 32 * per_row; i += THREADS) {
        const int row = i / per_row, cp = i - row * per_row, col = 8 * cp;
        const float *p = src(row);
        float x[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (p != nullptr) {
            if constexpr (VEC) {  // dim % 4 == 0, 16-byte aligned rows
#pragma unroll
                for (int v = 0; v < 2; ++v)
                    if (col + 4 * v < dim) {
                        const hf_v4f t = *reinterpret_cast<const hf_v4f *>(p + col + 4 * v);
                        x[4 * v] = t.x; x[4 * v + 1] = t.y; x[4 * v + 2] = t.z; x[4 * v + 3] = t.w;
                    }
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (col + e < dim) x[e] = p[col + e];
            }
        }
        const hf_v4f lo = {x[0], x[1], x[2], x[3]}, hi = {x[4], x[5], x[6], x[7]};
        A[(cp >> 1) * 64 + row + 32 * (cp & 1)] = hf_round8<TYPE>(lo, hi);
    }
}

// ================================================================================================ the walk
template <int TYPE, typename Epi>
__device__ __forceinline__ void ivf_walk(const hf_v4i *A, const hf_v4i *__restrict__ B, int64_t t_lo, int64_t t_hi, int ks, Epi epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t = t_lo + wave; t < t_hi; t += WAVES) {
        const hf_v4i *bt = B + t * ks * 64 + lane;
        hf_v16f acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        hf_v4i nb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) nb[u] = bt[u * 64];
        for (int s0 = 0; s0 < ks; s0 += 4) {  // ks is a multiple of 4; ascending k: one chain per output element
            hf_v4i a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                b[u] = nb[u];
                a[u] = A[(s0 + u) * 64 + lane];
            }
            if (s0 + 4 < ks) {
#pragma unroll
                for (int u = 0; u < 4; ++u) nb[u] = bt[(s0 + 4 + u) * 64];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = hf_mfma<TYPE>(a[u], b[u], acc);
        }
        epi(t, acc);
    }
}

__device__ __forceinline__ int ivf_row_of(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }
__device__ __forceinline__ bool ivf_better(float s, int c, float bs, int bc) { return s > bs || (s == bs && c < bc); }

// ================================================================================================ assign
struct IvfAssignArgs {
    const hf_v4i *cent;
    const float *rows;
    int64_t ld, n;
    int32_t *out_list;
    float *out_score;  // may be null
    int nlist, ks, dim;
};
template <int TYPE, bool VEC>
__global__ __launch_bounds__(THREADS) void srx_ivf_assign_kernel(IvfAssignArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ivf_lds[];
    hf_v4i *A = reinterpret_cast<hf_v4i *>(ivf_lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 31, h = lane >> 5;
    const int64_t r0 = (int64_t)blockIdx.x * 32;
    ivf_load_a<TYPE, VEC>(A, a.ks, a.dim, [&](int row) { return r0 + row < a.n ? a.rows + (r0 + row) * a.ld : nullptr; });
    __syncthreads();
    float bs[16];
    int bc[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        bs[reg] = -INFINITY;
        bc[reg] = 0;
    }
    ivf_walk<TYPE>(A, a.cent, 0, (a.nlist + 31) / 32, a.ks, [&](int64_t t, const hf_v16f &acc) {
        const int c = (int)t * 32 + r;
        if (c < a.nlist) {  // the last tile's padding rows are no centroids
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                if (ivf_better(acc[reg], c, bs[reg], bc[reg])) {
                    bs[reg] = acc[reg];
                    bc[reg] = c;
                }
        }
    });
#pragma unroll
    for (int reg = 0; reg < 16; ++reg)
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) {  // within the 32 lanes that hold one row
            const float os = __shfl_xor(bs[reg], off);
            const int oc = __shfl_xor(bc[reg], off);
            if (ivf_better(os, oc, bs[reg], bc[reg])) {
                bs[reg] = os;
                bc[reg] = oc;
            }
        }
    __syncthreads();  // every wave has left the walk: A's LDS is free
    float *red_s = reinterpret_cast<float *>(ivf_lds);
    int *red_c = reinterpret_cast<int *>(ivf_lds) + WAVES * 32;
    if (r == 0) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            red_s[wave * 32 + ivf_row_of(reg, h)] = bs[reg];
            red_c[wave * 32 + ivf_row_of(reg, h)] = bc[reg];
        }
    }
    __syncthreads();
    if (threadIdx.x < 32 && r0 + threadIdx.x < a.n) {
        float s = red_s[threadIdx.x];
        int c = red_c[threadIdx.x];
        for (int w = 1; w < WAVES; ++w)
            if (ivf_better(red_s[w * 32 + threadIdx.x], red_c[w * 32 + threadIdx.x], s, c)) {
                s = red_s[w * 32 + threadIdx.x];
                c = red_c[w * 32 + threadIdx.x];
            }
        a.out_list[r0 + threadIdx.x] = c;
        if (a.out_score != nullptr) a.out_score[r0 + threadIdx.x] = s;
    }
}

// ================================================================================================ probe
template <int TYPE>
__global__ __launch_bounds__(THREADS) void srx_ivf_centroid_scores_kernel(const hf_v4i *__restrict__ cent, int nlist, int ks,
                                                                          const float *__restrict__ queries, int nq, float *__restrict__ scores,
                                                                          int64_t ldc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ivf_lds[];
    hf_v4i *A = reinterpret_cast<hf_v4i *>(ivf_lds);
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * 32;
    ivf_load_a<TYPE, true>(A, ks, ks * 16, [&](int row) { return q0 + row < nq ? queries + (int64_t)(q0 + row) * (ks * 16) : nullptr; });
    __syncthreads();
    const int64_t n_ct = (nlist + 31) / 32;  // blockIdx.y: a slice of the centroid tiles (few queries: more workgroups than query blocks)
    ivf_walk<TYPE>(A, cent, n_ct * blockIdx.y / gridDim.y, n_ct * (blockIdx.y + 1) / gridDim.y, ks, [&](int64_t t, const hf_v16f &acc) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int q = q0 + ivf_row_of(reg, h);
            if (q < nq) scores[q * ldc + t * 32 + r] = acc[reg];  // column < ldc
        }
    });
}

// order-preserving 32-bit keys of fp32 scores (no score of a chain from +0.0f is -0.0f).  They use bit 31, which the selections of
// srx_common.h (keys below 2^31, 0 = none) do not take: the probe selects with a radix pass of its own.
__device__ __forceinline__ unsigned ivf_key(float x) {
    const unsigned u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : u | 0x80000000u;
}
__device__ __forceinline__ float ivf_unkey(unsigned key) { return __uint_as_float((key & 0x80000000u) ? key & 0x7FFFFFFFu : ~key); }

// one workgroup per query: T = the kk-th largest key by four 8-bit radix passes over the score row; every key above T and the
// lowest-numbered lists at T enter an LDS list of exactly kk entries, which is ranked by counting
__global__ __launch_bounds__(THREADS) void srx_ivf_probe_select_kernel(const float *__restrict__ scores, int64_t ldc, int nlist, int nprobe,
                                                                       int32_t *__restrict__ probe_list, float *__restrict__ probe_score) {
    __shared__ unsigned hist[256], lkey[IVF_MAX_PROBE];
    __shared__ int lid[IVF_MAX_PROBE], wsum[WAVES];
    __shared__ unsigned sh_digit, sh_need, sh_count;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;
    const int kk = nprobe < nlist ? nprobe : nlist;
    const float *row = scores + (int64_t)q * ldc;
    unsigned prefix = 0, mask = 0, need = (unsigned)kk;  // uniform
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[tid] = 0;  // THREADS == 256 bins
        __syncthreads();
        for (int c = tid; c < nlist; c += THREADS) {
            const unsigned key = ivf_key(row[c]);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid == 0) {  // the digit that holds the need-th largest of the keys under the prefix
            unsigned acc = 0;
            int b = 255;
            while (b > 0 && acc + hist[b] < need) acc += hist[b--];
            sh_digit = (unsigned)b;
            sh_need = need - acc;
            sh_count = 0;
        }
        __syncthreads();
        prefix |= sh_digit << shift;
        mask |= 255u << shift;
        need = sh_need;
        __syncthreads();
    }
    const unsigned T = prefix;  // `need` of the keys equal to T are taken, lowest lists first
    int ties_before = 0;         // uniform: keys == T in the chunks already walked
    for (int c0 = 0; c0 < nlist; c0 += THREADS) {
        const int c = c0 + tid;
        const unsigned key = c < nlist ? ivf_key(row[c]) : 0u;
        const bool tie = c < nlist && key == T;
        const unsigned long long bal = __ballot(tie);
        if (lane == 0) wsum[wave] = __popcll(bal);
        __syncthreads();
        int before = ties_before + __popcll(bal & ((1ull << lane) - 1ull)), all = 0;
        for (int w = 0; w < WAVES; ++w) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        if (c < nlist && (key > T || (tie && before < (int)need))) {
            const unsigned p = atomicAdd(&sh_count, 1u);  // < kk by construction
            lkey[p] = key;
            lid[p] = c;
        }
        ties_before += all;
        __syncthreads();
    }
    const int cnt = (int)sh_count;
    int32_t *ol = probe_list + (int64_t)q * nprobe;
    float *os = probe_score + (int64_t)q * nprobe;
    for (int i = tid; i < cnt; i += THREADS) {  // position = the entries that rank before this one
        const unsigned key = lkey[i];
        const int c = lid[i];
        int pos = 0;
        for (int j = 0; j < cnt; ++j) pos += (lkey[j] > key || (lkey[j] == key && lid[j] < c)) ? 1 : 0;
        ol[pos] = c;
        os[pos] = ivf_unkey(key);
    }
    for (int i = cnt + tid; i < nprobe; i += THREADS) {
        ol[i] = -1;
        os[i] = 0.0f;
    }
}

// ================================================================================================ update
struct IvfUpdateArgs {
    const float *rows;
    int64_t ld;
    const int64_t *member_ptr;
    const int32_t *member;
    const float *prev;
    float *out;
    int dim, col_blocks;
};
__global__ __launch_bounds__(THREADS) void srx_ivf_update_kernel(IvfUpdateArgs a) {
    __shared__ float part[WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x / a.col_blocks, col = (blockIdx.x - c * a.col_blocks) * 64 + lane;
    const bool live = col < a.dim;
    const int64_t m0 = a.member_ptr[c], m1 = a.member_ptr[c + 1];
    const int64_t cnt = m1 - m0;
    const int64_t o = (int64_t)c * a.dim + col;
    if (cnt <= 0) {  // uniform
        if (wave == 0 && live) a.out[o] = a.prev[o];
        return;
    }
    float total = 0.0f;  // wave 0's
    for (int64_t round0 = m0; round0 < m1; round0 += (int64_t)WAVES * IVF_CHUNK) {  // uniform: four chunks per round, one per wave
        const int64_t lo = round0 + (int64_t)wave * IVF_CHUNK;
        const int64_t hi = lo + IVF_CHUNK < m1 ? lo + IVF_CHUNK : m1;
        float s = 0.0f;
        int64_t i = lo;
        for (; i + 8 <= hi; i += 8) {  // eight rows in flight, added in member order
            float x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = live ? a.rows[(int64_t)a.member[i + u] * a.ld + col] : 0.0f;
#pragma unroll
            for (int u = 0; u < 8; ++u) s = s + x[u];
        }
        for (; i < hi; ++i) s = s + (live ? a.rows[(int64_t)a.member[i] * a.ld + col] : 0.0f);
        part[wave][lane] = s;
        __syncthreads();
        if (wave == 0) {
            for (int w = 0; w < WAVES; ++w)
                if (round0 + (int64_t)w * IVF_CHUNK < m1) total = total + part[w][lane];  // ascending chunk order, existing chunks only
        }
        __syncthreads();
    }
    if (wave == 0 && live) a.out[o] = total / (float)cnt;
}

// ================================================================================================ search: the pairs by list
__global__ __launch_bounds__(THREADS) void srx_ivf_zero_kernel(int32_t *p, int n) {
    const int i = blockIdx.x * THREADS + threadIdx.x;
    if (i < n) p[i] = 0;
}

// one workgroup per query: clean[q][j] = the list of slot j, or -1 for padding, a list outside [0, nlist) and a duplicate of an
// earlier slot; count[list] += 1 per kept pair
__global__ __launch_bounds__(THREADS) void srx_ivf_pairs_kernel(const int32_t *__restrict__ probe_list, int nprobe, int nlist,
                                                                int32_t *__restrict__ clean, int32_t *__restrict__ count) {
    __shared__ int L[IVF_MAX_PROBE];
    const int64_t base = (int64_t)blockIdx.x * nprobe;
    for (int j = threadIdx.x; j < nprobe; j += THREADS) L[j] = probe_list[base + j];
    __syncthreads();
    for (int j = threadIdx.x; j < nprobe; j += THREADS) {
        const int c = L[j];
        bool ok = c >= 0 && c < nlist;
        for (int i = 0; ok && i < j; ++i) ok = L[i] != c;
        clean[base + j] = ok ? c : -1;
        if (ok) atomicAdd(count + c, 1);
    }
}

// one workgroup: exclusive prefixes of the per-list pair counts and group counts (a group = up to 32 pairs of one list); fill = 0
__global__ __launch_bounds__(THREADS) void srx_ivf_offsets_kernel(const int32_t *__restrict__ count, int nlist, int32_t *__restrict__ pair_off,
                                                                  int32_t *__restrict__ grp_off, int32_t *__restrict__ fill) {
    __shared__ int sp[THREADS], sg[THREADS];
    const int tid = threadIdx.x, seg = (nlist + THREADS - 1) / THREADS;
    const int lo = min(tid * seg, nlist), hi = min(lo + seg, nlist);
    int p = 0, g = 0;
    for (int c = lo; c < hi; ++c) {
        p += count[c];
        g += (count[c] + 31) >> 5;
    }
    sp[tid] = p;
    sg[tid] = g;
    __syncthreads();
    if (tid == 0) {
        int ap = 0, ag = 0;
        for (int i = 0; i < THREADS; ++i) {
            const int tp = sp[i], tg = sg[i];
            sp[i] = ap;
            sg[i] = ag;
            ap += tp;
            ag += tg;
        }
    }
    __syncthreads();
    p = sp[tid];
    g = sg[tid];
    for (int c = lo; c < hi; ++c) {
        pair_off[c] = p;
        grp_off[c] = g;
        fill[c] = 0;
        p += count[c];
        g += (count[c] + 31) >> 5;
    }
    if (tid == THREADS - 1) {  // its segment ends the lists (or is empty behind them): p, g are the totals
        pair_off[nlist] = p;
        grp_off[nlist] = g;
    }
}

__global__ __launch_bounds__(THREADS) void srx_ivf_scatter_kernel(const int32_t *__restrict__ clean, int n_pairs, const int32_t *__restrict__ pair_off,
                                                                  int32_t *__restrict__ fill, int32_t *__restrict__ sorted) {
    const int p = blockIdx.x * THREADS + threadIdx.x;
    if (p >= n_pairs) return;
    const int c = clean[p];
    if (c >= 0) sorted[pair_off[c] + atomicAdd(fill + c, 1)] = p;  // the order inside a list decides only which group a pair joins
}

// ================================================================================================ search: the scan
struct IvfScanArgs {
    const hf_v4i *corpus;
    const float *queries;  // of the pass
    const int32_t *list_tile, *pair_off, *grp_off, *sorted;
    float *strips;         // [pair][max_list_tiles * 32]
    int64_t n_tiles, max_list_tiles;
    int nlist, nprobe, ks;
};
template <int TYPE>
__global__ __launch_bounds__(THREADS) void srx_ivf_scan_kernel(IvfScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char ivf_lds[];
    hf_v4i *A = reinterpret_cast<hf_v4i *>(ivf_lds);
    const int b = (int)blockIdx.x;
    if (b >= a.grp_off[a.nlist]) return;  // uniform: the grid is an upper bound of the groups
    int lo = 0, hi = a.nlist;             // the list c with grp_off[c] <= b < grp_off[c + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.grp_off[mid] <= b) lo = mid; else hi = mid;
    }
    const int c = lo;
    const int first = a.pair_off[c] + 32 * (b - a.grp_off[c]);
    const int live = min(32, a.pair_off[c + 1] - first);
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    ivf_load_a<TYPE, true>(A, a.ks, a.ks * 16, [&](int row) {
        return row < live ? a.queries + (int64_t)(a.sorted[first + row] / a.nprobe) * (a.ks * 16) : nullptr;
    });
    int64_t strip[16];  // the strips of this lane's 16 rows (< 0: no such pair)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = ivf_row_of(reg, h);
        strip[reg] = row < live ? (int64_t)a.sorted[first + row] * a.max_list_tiles * 32 : -1;
    }
    __syncthreads();
    const int64_t t_lo = max(a.list_tile[c], 0);
    const int64_t t_hi = min(min((int64_t)a.list_tile[c + 1], a.n_tiles), t_lo + a.max_list_tiles);
    const int64_t nt = t_hi > t_lo ? t_hi - t_lo : 0;  // blockIdx.y: a slice of the list's tiles (few groups: a long list is shared)
    ivf_walk<TYPE>(A, a.corpus, t_lo + nt * blockIdx.y / gridDim.y, t_lo + nt * (blockIdx.y + 1) / gridDim.y, a.ks, [&](int64_t t, const hf_v16f &acc) {
        const int64_t col = (t - t_lo) * 32 + r;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
            if (strip[reg] >= 0) a.strips[strip[reg] + col] = acc[reg];
    });
}

// one workgroup per (query, slot): the strip folded into an exact list of k (unordered) for the merge
struct IvfRankArgs {
    const float *strips;
    const int32_t *clean, *list_tile, *row_doc;
    const uint32_t *filter_bits;
    const int32_t *q_filter;
    int32_t *cand_doc;
    float *cand_score;
    int32_t *cand_count;
    int64_t n_tiles, max_list_tiles, n_docs, doc_base, filter_words;
    int nprobe, k, q0;
    float score_offset;
};
__global__ __launch_bounds__(THREADS) void srx_ivf_rank_kernel(IvfRankArgs a) {
    __shared__ MergeShared M;
    const int tid = threadIdx.x;
    const int64_t p = blockIdx.x;
    const int c = a.clean[p];
    if (c < 0) {  // uniform
        if (tid == 0) a.cand_count[p] = 0;
        return;
    }
    const int q = (int)(p / a.nprobe);
    const int64_t t_lo = max(a.list_tile[c], 0);
    const int64_t t_hi = min(min((int64_t)a.list_tile[c + 1], a.n_tiles), t_lo + a.max_list_tiles);
    const int64_t cols = t_hi > t_lo ? (t_hi - t_lo) * 32 : 0;
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
    const float *row = a.strips + p * a.max_list_tiles * 32;
    const int32_t *rdoc = a.row_doc + t_lo * 32;
    for (int64_t c0 = 0; c0 < cols; c0 += THREADS * IVF_NPT) {
        unsigned ubits[IVF_NPT];
        int udoc[IVF_NPT];
        const unsigned tau = M.tk.tau;
#pragma unroll
        for (int n = 0; n < IVF_NPT; ++n) {
            const int64_t col = c0 + n * THREADS + tid;
            float x = 0.0f;
            int doc = -1;
            if (col < cols) {
                doc = rdoc[col];
                x = row[col] + a.score_offset;
            }
            bool allowed = doc >= 0 && doc < a.n_docs;
            if (allowed && frow != nullptr) allowed = ((frow[doc >> 5] >> (doc & 31)) & 1u) != 0u;
            const unsigned bits = __float_as_uint(x);
            ubits[n] = (allowed && x > 0.0f && bits >= tau) ? bits : 0u;
            udoc[n] = (int)(a.doc_base + doc);
        }
        topk_fold<IVF_NPT, true>(ubits, udoc, a.k, M.tk, M.hist);
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

// ================================================================================================ host side
bool type_ok(int32_t type) { return type == SRX_HALF_F16 || type == SRX_HALF_BF16; }
inline int64_t r256(int64_t x) { return (x + 255) / 256 * 256; }

struct IvfPlan {
    int64_t ldc, strip_bytes;
    int P;  // queries per pass of a search
};
inline IvfPlan ivf_plan(int nq, int nlist, int nprobe, int64_t max_list_tiles) {
    IvfPlan p;
    p.ldc = (int64_t)((nlist + 31) / 32) * 32;
    p.strip_bytes = max_list_tiles * 128;
    int64_t qb = (1ll << 30) / ((int64_t)nprobe * p.strip_bytes);
    qb = qb < 1 ? 1 : qb > IVF_PASS ? IVF_PASS : qb;
    p.P = (int)(nq < qb ? nq : qb);
    return p;
}
struct IvfWs {
    float *cscores;  // [min(nq, 1024)][ldc]
    int32_t *probe_list, *clean, *sorted, *count, *fill, *pair_off, *grp_off;
    float *probe_score, *strips;
    srx_rows cand;
    void *merge;
    int64_t merge_bytes, bytes;
};
inline IvfWs ivf_ws(void *base, const IvfPlan &pl, int nq, int nlist, int nprobe, int k) {
    IvfWs w;
    char *p = (char *)base;
    auto take = [&](int64_t bytes) {
        char *r = p;
        p += r256(bytes);
        return r;
    };
    const int64_t N = (int64_t)pl.P * nprobe;
    w.cscores = (float *)take((int64_t)(nq < IVF_PASS ? nq : IVF_PASS) * pl.ldc * 4);
    w.probe_list = (int32_t *)take(N * 4);
    w.probe_score = (float *)take(N * 4);
    w.clean = (int32_t *)take(N * 4);
    w.sorted = (int32_t *)take(N * 4);
    w.count = (int32_t *)take((int64_t)(nlist + 1) * 4);
    w.fill = (int32_t *)take((int64_t)(nlist + 1) * 4);
    w.pair_off = (int32_t *)take((int64_t)(nlist + 1) * 4);
    w.grp_off = (int32_t *)take((int64_t)(nlist + 1) * 4);
    w.strips = (float *)take(N * pl.strip_bytes);
    int32_t *cd = (int32_t *)take(N * k * 4);
    float *cs = (float *)take(N * k * 4);
    w.cand = srx_plain_rows(cd, cs, (int32_t *)take(N * 4), k);
    w.merge_bytes = srx_merge_workspace_bytes(pl.P, nprobe, k);
    w.merge = p;
    p += w.merge_bytes;
    w.bytes = (int64_t)(p - (char *)base) + 256;
    return w;
}

int check_desc(const char *who, const srx_ivf_desc *d, int32_t nq, const float *queries, int32_t nprobe) {
    if (d == nullptr) return fail(SRX_ERR_INVALID, "%s: null desc", who);
    if (!type_ok(d->type)) return fail(SRX_ERR_INVALID, "%s: type must be SRX_HALF_F16 or SRX_HALF_BF16", who);
    if (!hf_dim_ok(d->dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 64, <= 1024 (pad the rows with zeros)", who);
    if (d->n_docs < 1 || d->n_docs > SRX_FILTER_MAX_DOCS) return fail(SRX_ERR_INVALID, "%s: n_docs out of range", who);
    if (d->nlist < 1 || d->nlist > IVF_MAX_LIST || d->nlist > d->n_docs) return fail(SRX_ERR_INVALID, "%s: need 1 <= nlist <= min(n_docs, 65536)", who);
    if (d->n_tiles < 1 || d->n_tiles > (1ll << 26)) return fail(SRX_ERR_INVALID, "%s: n_tiles out of range", who);
    if (d->max_list_tiles < 1 || d->max_list_tiles > d->n_tiles) return fail(SRX_ERR_INVALID, "%s: need 1 <= max_list_tiles <= n_tiles", who);
    if (d->doc_base < 0 || d->doc_base + d->n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: doc_base + n_docs must fit int32", who);
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if (nprobe < 1 || nprobe > d->nlist || nprobe > IVF_MAX_PROBE) return fail(SRX_ERR_INVALID, "%s: need 1 <= nprobe <= min(nlist, 1024)", who);
    if (nq > 0) {
        if (!d->corpus || !d->centroids || !d->list_tile || !d->row_doc) return fail(SRX_ERR_INVALID, "%s: desc holds a null pointer", who);
        if (!queries) return fail(SRX_ERR_INVALID, "%s: null queries", who);
        if (((uintptr_t)d->corpus | (uintptr_t)d->centroids) & 15) return fail(SRX_ERR_INVALID, "%s: corpus / centroids must be 16-byte aligned", who);
        if ((uintptr_t)queries & 15) return fail(SRX_ERR_INVALID, "%s: queries must be 16-byte aligned", who);
    }
    return SRX_OK;
}

}  // namespace

// the probe of one pass of <= 1024 queries (ivf_probe.h): shared with dense_ivfpq.hip, whose lists have the same centroids
int srx_ivf_probe_pass(const void *centroids, int nlist, int type, int dim_pad, const float *queries, int nq, int nprobe, int32_t *probe_list,
                       float *probe_score, float *cscores, int64_t ldc, hipStream_t stream) {
    const int ks = dim_pad / 16;
    const int qblocks = (nq + 31) / 32, n_ct = (nlist + 31) / 32;
    int slices = 512 / qblocks < n_ct / 4 ? 512 / qblocks : n_ct / 4;  // >= 512 workgroups while a slice keeps a tile per wave
    const dim3 grid((unsigned)qblocks, (unsigned)(slices < 1 ? 1 : slices));
    const size_t lds = (size_t)dim_pad * 64;
    if (type == SRX_HALF_F16)
        hipLaunchKernelGGL(srx_ivf_centroid_scores_kernel<SRX_HALF_F16>, grid, dim3(THREADS), lds, stream, (const hf_v4i *)centroids, nlist, ks, queries,
                           nq, cscores, ldc);
    else
        hipLaunchKernelGGL(srx_ivf_centroid_scores_kernel<SRX_HALF_BF16>, grid, dim3(THREADS), lds, stream, (const hf_v4i *)centroids, nlist, ks, queries,
                           nq, cscores, ldc);
    hipLaunchKernelGGL(srx_ivf_probe_select_kernel, dim3((unsigned)nq), dim3(THREADS), 0, stream, (const float *)cscores, ldc, nlist, nprobe, probe_list,
                       probe_score);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int srx_ivf_assign(int32_t device, int32_t type, const void *centroids_packed, int32_t nlist, int32_t dim, int32_t dim_pad,
                           const float *rows, int64_t ld, int64_t n, int32_t *out_list, float *out_score, void *stream_v) {
    const char *who = "srx_ivf_assign";
    if (!type_ok(type)) return fail(SRX_ERR_INVALID, "%s: type must be SRX_HALF_F16 or SRX_HALF_BF16", who);
    if (!hf_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 64, <= 1024", who);
    if (nlist < 1 || nlist > IVF_MAX_LIST) return fail(SRX_ERR_INVALID, "%s: need 1 <= nlist <= 65536", who);
    if (n < 0 || n > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: n out of range", who);
    if (dim < 1 || dim > dim_pad) return fail(SRX_ERR_INVALID, "%s: need 1 <= dim <= dim_pad", who);
    if (ld < dim) return fail(SRX_ERR_INVALID, "%s: need ld >= dim", who);
    if (n == 0) return SRX_OK;
    if (!centroids_packed || !rows || !out_list) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)rows & 3) return fail(SRX_ERR_INVALID, "%s: rows must be 4-byte aligned", who);
    if ((uintptr_t)centroids_packed & 15) return fail(SRX_ERR_INVALID, "%s: centroids must be 16-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    const IvfAssignArgs a = {(const hf_v4i *)centroids_packed, rows, ld, n, out_list, out_score, nlist, dim_pad / 16, dim};
    const bool vec = ((uintptr_t)rows & 15) == 0 && ld % 4 == 0 && dim % 4 == 0;
    const dim3 grid((unsigned)((n + 31) / 32));
    const size_t lds = (size_t)dim_pad * 64;
    hipStream_t stream = (hipStream_t)stream_v;
#define SRX_IVF_ASSIGN(T)                                                                                                       \
    if (vec)                                                                                                                    \
        hipLaunchKernelGGL((srx_ivf_assign_kernel<T, true>), grid, dim3(THREADS), lds, stream, a);                              \
    else                                                                                                                        \
        hipLaunchKernelGGL((srx_ivf_assign_kernel<T, false>), grid, dim3(THREADS), lds, stream, a);
    if (type == SRX_HALF_F16) {
        SRX_IVF_ASSIGN(SRX_HALF_F16)
    } else {
        SRX_IVF_ASSIGN(SRX_HALF_BF16)
    }
#undef SRX_IVF_ASSIGN
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int srx_ivf_update(int32_t device, const float *rows, int64_t ld, int32_t dim, int32_t nlist, const int64_t *member_ptr,
                           const int32_t *member, const float *prev_centroid, float *out_centroid, void *stream_v) {
    const char *who = "srx_ivf_update";
    if (nlist < 1 || nlist > IVF_MAX_LIST) return fail(SRX_ERR_INVALID, "%s: need 1 <= nlist <= 65536", who);
    if (dim < 1 || dim > 1024) return fail(SRX_ERR_INVALID, "%s: need 1 <= dim <= 1024", who);
    if (ld < dim) return fail(SRX_ERR_INVALID, "%s: need ld >= dim", who);
    if (!rows || !member_ptr || !member || !prev_centroid || !out_centroid) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)rows & 3) return fail(SRX_ERR_INVALID, "%s: rows must be 4-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    const int col_blocks = (dim + 63) / 64;
    const IvfUpdateArgs a = {rows, ld, member_ptr, member, prev_centroid, out_centroid, dim, col_blocks};
    hipLaunchKernelGGL(srx_ivf_update_kernel, dim3((unsigned)(nlist * col_blocks)), dim3(THREADS), 0, (hipStream_t)stream_v, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int64_t srx_ivf_workspace_bytes(int32_t nq, int32_t nlist, int32_t nprobe, int32_t k, int64_t max_list_tiles) {
    if (nq < 0 || nlist < 1 || nlist > IVF_MAX_LIST || nprobe < 1 || nprobe > nlist || nprobe > IVF_MAX_PROBE || k < 1 || k > KMAX ||
        max_list_tiles < 1 || max_list_tiles > (1ll << 26))
        return fail(SRX_ERR_INVALID, "srx_ivf_workspace_bytes: bad argument%s");
    return ivf_ws(nullptr, ivf_plan(nq, nlist, nprobe, max_list_tiles), nq, nlist, nprobe, k).bytes;
}

SRX_API int srx_ivf_probe(const srx_ivf_desc *desc, const float *queries, int32_t nq, int32_t nprobe, int32_t *probe_list, float *probe_score,
                          void *workspace, int64_t workspace_bytes, void *stream_v) {
    const char *who = "srx_ivf_probe";
    const int rc = check_desc(who, desc, nq, queries, nprobe);
    if (rc != SRX_OK) return rc;
    if (nq == 0) return SRX_OK;
    if (!probe_list || !probe_score) return fail(SRX_ERR_INVALID, "%s: null output", who);
    const int64_t ldc = (int64_t)((desc->nlist + 31) / 32) * 32;
    if (!workspace || workspace_bytes < r256((int64_t)(nq < IVF_PASS ? nq : IVF_PASS) * ldc * 4)) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    HIP_TRY(hipSetDevice(desc->device));
    for (int q0 = 0; q0 < nq; q0 += IVF_PASS) {
        const int qb = nq - q0 < IVF_PASS ? nq - q0 : IVF_PASS;
        const int prc = srx_ivf_probe_pass(desc->centroids, desc->nlist, desc->type, desc->dim_pad, queries + (int64_t)q0 * desc->dim_pad, qb, nprobe,
                                           probe_list + (int64_t)q0 * nprobe, probe_score + (int64_t)q0 * nprobe, (float *)workspace, ldc,
                                           (hipStream_t)stream_v);
        if (prc != SRX_OK) return prc;
    }
    return SRX_OK;
}

SRX_API int srx_ivf_search(const srx_ivf_desc *desc, const float *queries, int32_t nq, int32_t nprobe, int32_t k, const int32_t *probe_list,
                           const srx_doc_filter *filter, int32_t *out_doc, float *out_score, int32_t *out_count, void *workspace,
                           int64_t workspace_bytes, void *stream_v, float score_offset) {
    const char *who = "srx_ivf_search";
    int rc = check_desc(who, desc, nq, queries, nprobe);
    if (rc != SRX_OK) return rc;
    if (filter != nullptr) {
        rc = srx_check_filter(who, filter);
        if (rc != SRX_OK) return rc;
    }
    if (k < 1 || k > KMAX) return fail(SRX_ERR_INVALID, "%s: need 1 <= k <= 1024", who);
    if (nq == 0) return SRX_OK;
    if (!out_doc || !out_score || !out_count) return fail(SRX_ERR_INVALID, "%s: null output", who);
    const srx_ivf_desc &d = *desc;
    const IvfPlan pl = ivf_plan(nq, d.nlist, nprobe, d.max_list_tiles);
    const IvfWs w = ivf_ws(workspace, pl, nq, d.nlist, nprobe, k);
    if (!workspace || workspace_bytes < w.bytes) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    HIP_TRY(hipSetDevice(d.device));
    hipStream_t stream = (hipStream_t)stream_v;
    const int ks = d.dim_pad / 16;
    const size_t lds = (size_t)d.dim_pad * 64;
    for (int q0 = 0; q0 < nq; q0 += pl.P) {
        const int qb = nq - q0 < pl.P ? nq - q0 : pl.P;
        const int n_pairs = qb * nprobe;  // <= 2^20
        const float *qsrc = queries + (int64_t)q0 * d.dim_pad;
        const int32_t *plist = probe_list != nullptr ? probe_list + (int64_t)q0 * nprobe : w.probe_list;
        if (probe_list == nullptr) {
            rc = srx_ivf_probe_pass(d.centroids, d.nlist, d.type, d.dim_pad, qsrc, qb, nprobe, w.probe_list, w.probe_score, w.cscores, pl.ldc, stream);
            if (rc != SRX_OK) return rc;
        }
        hipLaunchKernelGGL(srx_ivf_zero_kernel, dim3((unsigned)((d.nlist + THREADS) / THREADS)), dim3(THREADS), 0, stream, w.count, d.nlist + 1);
        hipLaunchKernelGGL(srx_ivf_pairs_kernel, dim3((unsigned)qb), dim3(THREADS), 0, stream, plist, nprobe, d.nlist, w.clean, w.count);
        hipLaunchKernelGGL(srx_ivf_offsets_kernel, dim3(1), dim3(THREADS), 0, stream, (const int32_t *)w.count, d.nlist, w.pair_off, w.grp_off, w.fill);
        hipLaunchKernelGGL(srx_ivf_scatter_kernel, dim3((unsigned)((n_pairs + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream,
                           (const int32_t *)w.clean, n_pairs, (const int32_t *)w.pair_off, w.fill, w.sorted);
        // groups <= lists that hold a pair + pairs / 32
        const unsigned groups_max = (unsigned)((d.nlist < n_pairs ? d.nlist : n_pairs) + n_pairs / 32);
        const IvfScanArgs sa = {(const hf_v4i *)d.corpus, qsrc, d.list_tile, w.pair_off, w.grp_off, w.sorted, w.strips, d.n_tiles, d.max_list_tiles,
                                d.nlist, nprobe, ks};
        const unsigned slices = 1024u / groups_max < 1u ? 1u : 1024u / groups_max > 16u ? 16u : 1024u / groups_max;  // of a list's tiles, while groups are few
        if (d.type == SRX_HALF_F16)
            hipLaunchKernelGGL(srx_ivf_scan_kernel<SRX_HALF_F16>, dim3(groups_max, slices), dim3(THREADS), lds, stream, sa);
        else
            hipLaunchKernelGGL(srx_ivf_scan_kernel<SRX_HALF_BF16>, dim3(groups_max, slices), dim3(THREADS), lds, stream, sa);
        const IvfRankArgs ra = {w.strips, w.clean, d.list_tile, d.row_doc, filter ? filter->bits : nullptr, filter ? filter->q_filter : nullptr,
                                w.cand.doc, w.cand.score, w.cand.count, d.n_tiles, d.max_list_tiles, d.n_docs, d.doc_base,
                                srx_filter_row_words(d.n_docs), nprobe, k, q0, score_offset};
        hipLaunchKernelGGL(srx_ivf_rank_kernel, dim3((unsigned)n_pairs), dim3(THREADS), 0, stream, ra);
        HIP_TRY(hipGetLastError());
        const srx_rows out = srx_plain_rows(out_doc + (int64_t)q0 * k, out_score + (int64_t)q0 * k, out_count + q0, k);
        rc = srx_merge_impl(d.device, w.cand, qb, nprobe, k, 0, out, w.merge, w.merge_bytes, stream_v);
        if (rc != SRX_OK) return rc;
    }
    return SRX_OK;
}
