// facets.hip -- facet counts (sparse_rx_facets.h): per output row (a filter row, or a result list) the number of its docs in
// every bin of one resident metadata column, plus {missing, other, total}.
//
// Replaces nothing in the reference project: it does not aggregate results.
//
// Both kernels count into a private histogram in LDS (u32[1024] or u32[8192], two instances per binning kind) and share one
// binning function per mode (fc_bin_codes, fc_bin_edges, fc_label_mask), one wave-level add (fc_hist_add / fc_labels_add).
//
// Row form.  A wave's UNIT is the row words of `unit_lanes` lanes, 16 bytes each: 64 lanes = 256 words = 8192 docs, 1 KB
// contiguous per wave; a SMALL call (fewer than FC_TARGET_WGS pairs of a row and a 2048-doc chunk) takes 32, 16, 8 or 4 lanes
// (4096 .. 512 docs), so that its docs spread over more waves (the rule is in srx_facet_counts).  A workgroup's CHUNK is its four waves'
// units, and a workgroup walks a SEGMENT of seg_chunks chunks for one row before it flushes.  Inside a unit the wave first
// ballots which lanes hold a set bit: a unit without one costs its load and nothing else.  For every PAIR of lanes with a bit (256 docs = 4 steps of 64 docs) the
// eight words come to scalar registers by v_readlane, and in step t lane l looks at doc d0 + 64 t + l: its bit, its validity
// bit, and -- only where both are set -- its value, one contiguous column load per step, the four of a pair in flight together.
// A step whose 64 bits are zero is skipped (a uniform branch).  total / missing / other are popcounts of scalar masks.
//
// Hot bins.  fc_hist_add takes up to FC_PEEL_TRIES leaders among the lanes that count: the lanes with the leader's bin are found
// with one ballot, and when they are FC_PEEL_MIN or more the leader adds their number with ONE LDS atomic; the rest add 1
// each.  With 90 % of the docs in one value the hot bin is peeled in the first try 9 times of 10; with uniform values the
// tries cost three ballots per step and the adds hit different banks.  LABELS: lane i keeps the count of label i in a
// register (a ballot per label and step) and adds it to LDS once per row.
//
// Flush.  After a row's segment the non-zero bins go to out_counts with global integer adds and are re-zeroed in the same pass;
// a (segment, row) that counted nothing skips the pass.  The segment is at least FC_FLUSH_RATIO * n_bins docs (flushed words
// are at most 1 / 16 of the docs scanned; 1 / 2 in a call too small to fill the chip, where the flush is not what costs), and
// grows with n_rows so that the grid stays near FC_TARGET_WGS workgroups.  Flushed words never exceed the docs counted.  The
// outputs are zeroed by two hipMemsetAsync on the stream before the launch.
//
// Rows of one segment are consecutive blocks (the dispatch order of fields.hip): they read the same column values, which come
// from HBM once and from L2 afterwards.  EDGES with at most 1024 bins keep the edges in LDS; above that the bisection reads
// them from global memory (cached, 64 KB at most).
//
// List form.  One workgroup per list, the live rule of collapse.hip, gathered values, the same adds; the workgroup owns its
// output row and stores it: no global atomics.
//
// The checks of the column and of n_docs / doc_base and the column helpers are field_common.h's; the list form keeps its list checks (nq before m, no cap).
#include "field_common.h"
#include "sparse_rx_facets.h"

namespace {

constexpr int FC_LANE_DOCS = 128;                     // docs of one lane's 16 bytes of row words
constexpr int FC_MIN_LANES = 4, FC_MAX_LANES = 64;    // lanes of a wave's unit: 512 .. 8192 docs, a chunk 2048 .. 32768
constexpr int FC_SMALL_BINS = 1024;                   // the small histogram instance (and edges in LDS)
constexpr int FC_FLUSH_RATIO = 16;                    // a segment scans at least 16 docs per bin it may flush ...
constexpr int FC_FLUSH_RATIO_SMALL = 2;               // ... 2 in a call that cannot fill the chip
constexpr int FC_TARGET_WGS = 2048;                   // workgroups a launch aims at (256 CUs x 8)
constexpr int FC_MAX_ROWS_Y = 65535;                  // grid.y; more rows than that are looped over
constexpr int FC_PEEL_TRIES = 3, FC_PEEL_MIN = 4;     // fc_hist_add

enum { K_CODES_I32 = 0, K_CODES_I64 = 1, K_LABELS = 2, K_EDGES_I32 = 3, K_EDGES_I64 = 4, K_EDGES_F32 = 5 };

struct FacetArgs {
    const void *data;            // the column
    const uint32_t *valid;       // one filter row, or null
    const int64_t *edges;        // EDGES: i64[n_bins + 1]
    int64_t origin;              // CODES
    int32_t *out_counts;         // [rows][n_bins]
    int32_t *out_extra;          // [rows][3]
    int64_t n_docs, words;
    const uint32_t *base_bits;   // row form: null = every doc
    const int32_t *base_q;       // row form: null = base row 0
    const int32_t *cand_doc;     // list form: [nq][m]
    const int32_t *cand_count;   // list form: [nq] or null
    int64_t doc_base;            // list form
    int n_bins, n_rows, seg_chunks, n_chunks, m;
    int unit_lanes;              // row form: lanes of a wave's unit (a power of two in 4 .. 64)
};

template <int KIND>
__device__ __forceinline__ int64_t fc_load(const void *data, uint32_t d) {
    constexpr bool f32 = KIND == K_EDGES_F32;
    return srx_field_load(data, !f32 && KIND != K_CODES_I32 && KIND != K_EDGES_I32, f32, d);
}

// ---- the binning functions: one per mode, shared by both kernels (tests/facets_ref.py restates them)
__device__ __forceinline__ int fc_bin_codes(int64_t v, int64_t origin, int n_bins) {
    const uint64_t off = (uint64_t)v - (uint64_t)origin;  // exact for v >= origin: the difference lies in [0, 2^64)
    return v >= origin && off < (uint64_t)n_bins ? (int)off : -1;
}

// (number of j in [0, n_bins] with edges[j] <= v) - 1 by bisection over ascending edges; -1 = no bin
template <bool F32>
__device__ __forceinline__ int fc_bin_edges(int64_t v, const int64_t *edges, int n_bins) {
    int lo = 0, hi = n_bins + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;  // < n_bins + 1: inside the array
        const int64_t e = edges[mid];
        const bool le = F32 ? __int_as_float((int)e) <= __int_as_float((int)v) : e <= v;  // a NaN value: never
        if (le) lo = mid + 1; else hi = mid;
    }
    return lo - 1 < n_bins ? lo - 1 : -1;
}

__device__ __forceinline__ uint64_t fc_label_mask(int n_bins) { return n_bins >= 64 ? ~0ull : (1ull << n_bins) - 1ull; }

template <int KIND>
__device__ __forceinline__ int fc_bin(int64_t v, const FacetArgs &a, const int64_t *edges) {
    if constexpr (KIND == K_CODES_I32 || KIND == K_CODES_I64) return fc_bin_codes(v, a.origin, a.n_bins);
    else return fc_bin_edges<KIND == K_EDGES_F32>(v, edges, a.n_bins);
}

// ---- the wave's adds
// hist[bin] += 1 for every lane with `in` (0 <= bin < n_bins there).  Lanes that share a bin with one of up to FC_PEEL_TRIES
// leaders are added by the leader in one atomic when they are FC_PEEL_MIN or more.
__device__ __forceinline__ void fc_hist_add(uint32_t *hist, bool in, int bin, int lane) {
    uint64_t rem = __ballot(in), plain = 0;
    for (int t = 0; t < FC_PEEL_TRIES && rem != 0; ++t) {
        const int lead = __ffsll((unsigned long long)rem) - 1;
        const int b = __builtin_amdgcn_readlane(bin, lead);
        const uint64_t same = __ballot(in && bin == b);  // a subset of rem: the lanes taken out before hold other bins
        const int n = __popcll(same);
        if (n >= FC_PEEL_MIN) {
            if (lane == lead) atomicAdd(&hist[b], (uint32_t)n);
        } else {
            plain |= same;
        }
        rem &= ~same;
    }
    plain |= rem;
    if ((plain >> lane) & 1ull) atomicAdd(&hist[bin], 1u);
}

// lane i keeps the count of label i: acc += lanes with `in` and bit i of vm
__device__ __forceinline__ void fc_labels_add(uint32_t &acc, bool in, uint64_t vm, int n_bins, int lane) {
    if (__ballot(in && vm != 0) == 0ull) return;
    for (int i = 0; i < n_bins; ++i) {
        const int c = __popcll(__ballot(in && ((vm >> i) & 1ull)));
        acc += lane == i ? (uint32_t)c : 0u;
    }
}

// one step of 64 positions: lane `lane` holds a doc that has the value v iff `has`
template <int KIND>
__device__ __forceinline__ void fc_count(const FacetArgs &a, const int64_t *edges, uint32_t *hist, uint32_t &lacc, unsigned &other, bool has,
                                         int64_t v, int lane) {
    if constexpr (KIND == K_LABELS) {
        const uint64_t vm = has ? (uint64_t)v & fc_label_mask(a.n_bins) : 0ull;
        other += (unsigned)__popcll(__ballot(has && vm == 0ull));
        fc_labels_add(lacc, has, vm, a.n_bins, lane);
    } else {
        int bin = -1;
        if (has) bin = fc_bin<KIND>(v, a, edges);
        other += (unsigned)__popcll(__ballot(has && bin < 0));
        fc_hist_add(hist, has && bin >= 0, bin, lane);
    }
}

template <int KIND, int CAP>
struct FacetShared {
    static constexpr bool LDS_EDGES = KIND >= K_EDGES_I32 && CAP == FC_SMALL_BINS;
    uint32_t hist[CAP];
    int64_t edges[LDS_EDGES ? CAP + 1 : 1];
    uint32_t extra[4];
};

// zero the histogram, stage the edges; returns where the bisection reads them
template <int KIND, int CAP>
__device__ __forceinline__ const int64_t *fc_prepare(FacetShared<KIND, CAP> &S, const FacetArgs &a, int tid) {
    for (int b = tid; b < a.n_bins; b += THREADS) S.hist[b] = 0u;  // n_bins <= CAP
    if (tid < 4) S.extra[tid] = 0u;
    const int64_t *edges = a.edges;
    if constexpr (FacetShared<KIND, CAP>::LDS_EDGES) {
        for (int j = tid; j <= a.n_bins; j += THREADS) S.edges[j] = a.edges[j];
        edges = S.edges;
    }
    __syncthreads();
    return edges;
}

template <int KIND, int CAP>
__global__ __launch_bounds__(THREADS) void srx_facet_rows_kernel(FacetArgs a) {
    __shared__ FacetShared<KIND, CAP> S;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t *edges = fc_prepare<KIND, CAP>(S, a, tid);
    // consecutive blocks are the rows of one segment: they share its column values in L2
    const uint64_t order = blockIdx.x + (uint64_t)gridDim.x * blockIdx.y;
    const int seg = (int)(order / gridDim.y), row0 = (int)(order % gridDim.y);
    const int chunk0 = seg * a.seg_chunks;
    const int chunk1 = chunk0 + a.seg_chunks < a.n_chunks ? chunk0 + a.seg_chunks : a.n_chunks;
    for (int r = row0; r < a.n_rows; r += gridDim.y) {
        const int br = srx_filter_base_row(a.base_bits, a.base_q, r);
        const uint32_t *brow = br >= 0 ? a.base_bits + (int64_t)br * a.words : nullptr;
        unsigned total = 0, missing = 0, other = 0;  // wave-uniform
        uint32_t lacc = 0;
        for (int c = chunk0; c < chunk1; ++c) {
            const int64_t w_unit = ((int64_t)c * WAVES + wave) * (a.unit_lanes * 4);
            const int64_t w_lane = w_unit + 4 * lane;
            uint4 acc = make_uint4(0u, 0u, 0u, 0u);
            const bool inside = lane < a.unit_lanes && w_lane < a.words;  // words is a multiple of 4: a lane's 16 bytes are inside or outside as a whole
            if (inside) {
                acc = make_uint4(srx_filter_word_docs(a.n_docs, w_lane * 32), srx_filter_word_docs(a.n_docs, w_lane * 32 + 32),
                                 srx_filter_word_docs(a.n_docs, w_lane * 32 + 64), srx_filter_word_docs(a.n_docs, w_lane * 32 + 96));
                if (brow != nullptr) {
                    const uint4 bw = srx_field_row_words(brow, w_lane);
                    acc.x &= bw.x, acc.y &= bw.y, acc.z &= bw.z, acc.w &= bw.w;
                }
            }
            const uint64_t nz = __ballot((acc.x | acc.y | acc.z | acc.w) != 0u);
            if (nz == 0ull) continue;
            uint4 ok = make_uint4(~0u, ~0u, ~0u, ~0u);
            if (a.valid != nullptr && inside) ok = srx_field_row_words(a.valid, w_lane);
            uint64_t pairs = (nz | (nz >> 1)) & 0x5555555555555555ull;  // bit 2 p: lane 2 p or 2 p + 1 holds a doc
            while (pairs != 0ull) {
                const int j = __ffsll((unsigned long long)pairs) - 1;  // even: j + 1 <= 63
                pairs &= pairs - 1ull;
                uint64_t m[4], h[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const int src = j + (t >> 1);
                    const uint32_t m_lo = (uint32_t)__builtin_amdgcn_readlane((int)((t & 1) ? acc.z : acc.x), src);
                    const uint32_t m_hi = (uint32_t)__builtin_amdgcn_readlane((int)((t & 1) ? acc.w : acc.y), src);
                    const uint32_t h_lo = (uint32_t)__builtin_amdgcn_readlane((int)((t & 1) ? ok.z : ok.x), src);
                    const uint32_t h_hi = (uint32_t)__builtin_amdgcn_readlane((int)((t & 1) ? ok.w : ok.y), src);
                    m[t] = (uint64_t)m_lo | ((uint64_t)m_hi << 32);
                    h[t] = (uint64_t)h_lo | ((uint64_t)h_hi << 32);
                }
                const uint32_t d0 = (uint32_t)(w_unit * 32) + 128u * (uint32_t)j + (uint32_t)lane;
                bool has[4];
                int64_t v[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {  // a set bit of m lies below n_docs: the load is inside the column
                    has[t] = ((m[t] & h[t]) >> lane) & 1ull;
                    v[t] = 0;
                    if (has[t]) v[t] = fc_load<KIND>(a.data, d0 + 64u * t);
                }
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    if (m[t] == 0ull) continue;
                    total += (unsigned)__popcll(m[t]);
                    missing += (unsigned)__popcll(m[t] & ~h[t]);
                    fc_count<KIND>(a, edges, S.hist, lacc, other, has[t], v[t], lane);
                }
            }
        }
        if constexpr (KIND == K_LABELS) {
            if (lane < a.n_bins && lacc != 0u) atomicAdd(&S.hist[lane], lacc);
        }
        if (lane == 0 && total != 0u) {  // the waves' three sums meet in LDS: one global add each per (segment, row)
            atomicAdd(&S.extra[0], missing);
            atomicAdd(&S.extra[1], other);
            atomicAdd(&S.extra[2], total);
        }
        if (__syncthreads_or(total != 0u)) {  // else: nothing counted, the histogram is still zero
            int32_t *out = a.out_counts + (int64_t)r * a.n_bins;
            for (int b = tid; b < a.n_bins; b += THREADS) {
                const uint32_t cnt = S.hist[b];
                if (cnt != 0u) {
                    atomicAdd(out + b, (int32_t)cnt);
                    S.hist[b] = 0u;
                }
            }
            if (tid < 3) {
                const uint32_t x = S.extra[tid];
                if (x != 0u) atomicAdd(a.out_extra + (int64_t)r * 3 + tid, (int32_t)x);
                S.extra[tid] = 0u;
            }
            __syncthreads();  // the zeros before the next row's adds
        }
    }
}

template <int KIND, int CAP>
__global__ __launch_bounds__(THREADS) void srx_facet_lists_kernel(FacetArgs a) {
    __shared__ FacetShared<KIND, CAP> S;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t *edges = fc_prepare<KIND, CAP>(S, a, tid);
    const int64_t q = blockIdx.x;
    const int m = a.m;
    int n = a.cand_count != nullptr ? cload_i32(a.cand_count + q) : m;  // the live prefix of the list
    n = n < 0 ? 0 : n > m ? m : n;
    const int32_t *row_doc = a.cand_doc + q * m;
    unsigned total = 0, missing = 0, other = 0;  // wave-uniform
    uint32_t lacc = 0;
    for (int64_t i0 = (int64_t)wave * 64; i0 < n; i0 += THREADS) {  // 64 bits: i0 + THREADS may pass 2^31
        const int64_t i = i0 + lane;
        bool on = false, has = false;
        int64_t v = 0;
        if (i < n) {  // i < n <= m: inside the row
            const int64_t local = (int64_t)gload_i32(row_doc + i) - a.doc_base;
            if (local >= 0 && local < a.n_docs) {
                on = has = true;
                if (a.valid != nullptr) has = srx_field_valid_bit(a.valid, local);
                if (has) v = fc_load<KIND>(a.data, (uint32_t)local);
            }
        }
        const uint64_t live = __ballot(on);
        if (live == 0ull) continue;
        total += (unsigned)__popcll(live);
        missing += (unsigned)__popcll(__ballot(on && !has));
        fc_count<KIND>(a, edges, S.hist, lacc, other, has, v, lane);
    }
    if constexpr (KIND == K_LABELS) {
        if (lane < a.n_bins && lacc != 0u) atomicAdd(&S.hist[lane], lacc);
    }
    if (lane == 0 && total != 0u) {
        atomicAdd(&S.extra[0], missing);
        atomicAdd(&S.extra[1], other);
        atomicAdd(&S.extra[2], total);
    }
    __syncthreads();
    int32_t *out = a.out_counts + q * a.n_bins;
    for (int b = tid; b < a.n_bins; b += THREADS) out[b] = (int32_t)S.hist[b];
    if (tid < 3) a.out_extra[q * 3 + tid] = (int32_t)S.extra[tid];
}

// what both entry points check of the column and the bins; the binning kind (K_*) or a negative code
int check_col_bins(const char *who, const srx_field_col *col, int64_t n_docs, const srx_facet_bins *bins) {
    if (!col) return fail(SRX_ERR_INVALID, "%s: null col", who);
    int rc = srx_check_field_cols(who, col, 1, SRX_FIELD_TYPES_ALL, nullptr);
    if (rc == SRX_OK) rc = srx_check_field_docs(who, n_docs, 0, false);  // doc_base comes behind the bins (srx_facet_counts_lists)
    if (rc != SRX_OK) return rc;
    const int t = col->type;
    if (!bins) return fail(SRX_ERR_INVALID, "%s: null bins", who);
    const int mode = bins->mode;
    if (mode != SRX_FACET_CODES && mode != SRX_FACET_LABELS && mode != SRX_FACET_EDGES) return fail(SRX_ERR_INVALID, "%s: unknown bins mode", who);
    if (mode == SRX_FACET_CODES && t != SRX_FIELD_I32 && t != SRX_FIELD_I64) return fail(SRX_ERR_INVALID, "%s: SRX_FACET_CODES is for I32 and I64 columns", who);
    if (mode == SRX_FACET_LABELS && t != SRX_FIELD_SET64) return fail(SRX_ERR_INVALID, "%s: SRX_FACET_LABELS is for SET64 columns", who);
    if (mode == SRX_FACET_EDGES && t == SRX_FIELD_SET64) return fail(SRX_ERR_INVALID, "%s: SRX_FACET_EDGES is for I32, I64 and F32 columns", who);
    if (mode == SRX_FACET_LABELS) {
        if (bins->n_bins < 1 || bins->n_bins > 64) return fail(SRX_ERR_INVALID, "%s: n_bins must be in [1, 64] for SRX_FACET_LABELS", who);
        return K_LABELS;
    }
    if (bins->n_bins < 1 || bins->n_bins > SRX_FACET_MAX_BINS) return fail(SRX_ERR_INVALID, "%s: n_bins must be in [1, 8192]", who);
    if (mode == SRX_FACET_CODES) return t == SRX_FIELD_I32 ? K_CODES_I32 : K_CODES_I64;
    if (!bins->edges) return fail(SRX_ERR_INVALID, "%s: null edges", who);
    if ((uintptr_t)bins->edges & 7) return fail(SRX_ERR_INVALID, "%s: edges must be 8-byte aligned", who);
    return t == SRX_FIELD_I32 ? K_EDGES_I32 : t == SRX_FIELD_I64 ? K_EDGES_I64 : K_EDGES_F32;
}

template <int KIND>
void launch_kind(bool lists, const dim3 &grid, hipStream_t stream, const FacetArgs &a) {
    const bool small = a.n_bins <= FC_SMALL_BINS;
    if (lists) {
        if (small) hipLaunchKernelGGL((srx_facet_lists_kernel<KIND, FC_SMALL_BINS>), grid, dim3(THREADS), 0, stream, a);
        else hipLaunchKernelGGL((srx_facet_lists_kernel<KIND, SRX_FACET_MAX_BINS>), grid, dim3(THREADS), 0, stream, a);
    } else {
        if (small) hipLaunchKernelGGL((srx_facet_rows_kernel<KIND, FC_SMALL_BINS>), grid, dim3(THREADS), 0, stream, a);
        else hipLaunchKernelGGL((srx_facet_rows_kernel<KIND, SRX_FACET_MAX_BINS>), grid, dim3(THREADS), 0, stream, a);
    }
}

void launch(int kind, bool lists, const dim3 &grid, hipStream_t stream, const FacetArgs &a) {
    switch (kind) {
        case K_CODES_I32: launch_kind<K_CODES_I32>(lists, grid, stream, a); break;
        case K_CODES_I64: launch_kind<K_CODES_I64>(lists, grid, stream, a); break;
        case K_LABELS: launch_kind<K_LABELS>(lists, grid, stream, a); break;  // n_bins <= 64: the small instance
        case K_EDGES_I32: launch_kind<K_EDGES_I32>(lists, grid, stream, a); break;
        case K_EDGES_I64: launch_kind<K_EDGES_I64>(lists, grid, stream, a); break;
        default: launch_kind<K_EDGES_F32>(lists, grid, stream, a); break;
    }
}

}  // namespace

SRX_API int srx_facet_counts(int32_t device, const srx_field_col *col, int64_t n_docs, const srx_facet_bins *bins, const srx_doc_filter *filter,
                             int32_t n_rows, int32_t *out_counts, int32_t *out_extra, void *stream_v) {
    const char *who = "srx_facet_counts";
    const int kind = check_col_bins(who, col, n_docs, bins);
    if (kind < 0) return kind;
    if (n_rows < 0) return fail(SRX_ERR_INVALID, "%s: n_rows < 0", who);
    if (filter) {
        const int rc = srx_check_filter(who, filter);
        if (rc != SRX_OK) return rc;
    }
    if (n_rows == 0) return SRX_OK;
    if (!out_counts || !out_extra) return fail(SRX_ERR_INVALID, "%s: null out_counts / out_extra", who);
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    FacetArgs a;
    memset(&a, 0, sizeof(a));
    a.data = col->data, a.valid = col->valid;
    a.edges = bins->edges, a.origin = bins->origin, a.n_bins = bins->n_bins;
    a.out_counts = out_counts, a.out_extra = out_extra;
    a.n_docs = n_docs, a.words = srx_filter_row_words(n_docs);
    a.base_bits = filter ? filter->bits : nullptr;
    a.base_q = filter ? filter->q_filter : nullptr;
    a.n_rows = n_rows;
    // The launch rule.  A call is SMALL when even chunks of the smallest unit cannot fill the chip: what it costs is the chain of
    // rounds one wave walks, not bytes or flushes.  It flushes after 2 docs per bin instead of 16, and its unit halves from 64 lanes
    // while a chunk is still longer than that shortest segment (below that a smaller unit adds no workgroup).  Any other call keeps
    // 64 lanes: more, smaller workgroups there only add flushes onto the same output words (measured: one row of 10 M docs over 64
    // values took 0.147 ms dense and 0.092 ms sparse with 1 024-doc units against 0.125 and 0.042 ms with 8 192-doc units).
    const auto chunks_of = [n_docs](int lanes) { return (n_docs + (int64_t)WAVES * lanes * FC_LANE_DOCS - 1) / ((int64_t)WAVES * lanes * FC_LANE_DOCS); };
    const bool small = chunks_of(FC_MIN_LANES) * n_rows < FC_TARGET_WGS;
    const int64_t seg_docs = (int64_t)(small ? FC_FLUSH_RATIO_SMALL : FC_FLUSH_RATIO) * a.n_bins;
    int lanes = FC_MAX_LANES;
    while (small && lanes > FC_MIN_LANES && (int64_t)WAVES * lanes * FC_LANE_DOCS > seg_docs) lanes >>= 1;
    a.unit_lanes = lanes;
    const int64_t chunk_docs = (int64_t)WAVES * lanes * FC_LANE_DOCS;
    a.n_chunks = (int)chunks_of(lanes);  // <= 2^20
    // the flush rule: a segment scans at least seg_docs, and as many chunks as keep the grid near FC_TARGET_WGS
    const int64_t least = (seg_docs + chunk_docs - 1) / chunk_docs;
    const int64_t spread = (int64_t)a.n_chunks * n_rows / FC_TARGET_WGS;
    int64_t seg = least > spread ? least : spread;
    seg = seg < 1 ? 1 : seg > a.n_chunks ? a.n_chunks : seg;
    a.seg_chunks = (int)seg;
    const unsigned n_seg = (unsigned)((a.n_chunks + a.seg_chunks - 1) / a.seg_chunks);
    HIP_TRY(hipMemsetAsync(out_counts, 0, (size_t)n_rows * a.n_bins * sizeof(int32_t), stream));
    HIP_TRY(hipMemsetAsync(out_extra, 0, (size_t)n_rows * 3 * sizeof(int32_t), stream));
    launch(kind, false, dim3(n_seg, (unsigned)(n_rows < FC_MAX_ROWS_Y ? n_rows : FC_MAX_ROWS_Y)), stream, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int srx_facet_counts_lists(int32_t device, const srx_field_col *col, int64_t n_docs, int64_t doc_base, const srx_facet_bins *bins,
                                   const int32_t *cand_doc, const int32_t *cand_count, int32_t nq, int32_t m, int32_t *out_counts,
                                   int32_t *out_extra, void *stream_v) {
    const char *who = "srx_facet_counts_lists";
    const int kind = check_col_bins(who, col, n_docs, bins);
    if (kind < 0) return kind;
    const int rc = srx_check_field_docs(who, n_docs, doc_base, true);  // n_docs is checked: what is left is doc_base and the bound
    if (rc != SRX_OK) return rc;
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if (m < 1) return fail(SRX_ERR_INVALID, "%s: m must be >= 1", who);
    if ((int64_t)nq * m > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: nq * m must not exceed 2^31 - 1", who);
    if (nq == 0) return SRX_OK;
    if (!cand_doc) return fail(SRX_ERR_INVALID, "%s: null cand_doc", who);
    if (!out_counts || !out_extra) return fail(SRX_ERR_INVALID, "%s: null out_counts / out_extra", who);
    HIP_TRY(hipSetDevice(device));
    FacetArgs a;
    memset(&a, 0, sizeof(a));
    a.data = col->data, a.valid = col->valid;
    a.edges = bins->edges, a.origin = bins->origin, a.n_bins = bins->n_bins;
    a.out_counts = out_counts, a.out_extra = out_extra;
    a.n_docs = n_docs, a.words = srx_filter_row_words(n_docs);
    a.cand_doc = cand_doc, a.cand_count = cand_count, a.doc_base = doc_base, a.m = m;
    launch(kind, true, dim3((unsigned)nq), (hipStream_t)stream_v, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
