// maxsim_search.hip -- late-interaction search (include/late/sparse_rx_maxsim_search.h): the k docs of the WHOLE token store with
// the best MaxSim score per query.  Replaces nothing in the reference project: it has no multi-vector index.  Same build flags as
// the other units; -ffp-contract=off is part of the contract (every add of the ordered sum is rounded on its own).  The scores are
// the reranker's (maxsim.hip) bit for bit; the kernels are not: the reranker GATHERS the docs of a list, one wave per (query, doc),
// every query reading the doc's token rows again; the search STREAMS the packed store once per group of queries.
//
//   pack    the reranker's kernel (maxsim_common.h): the call's f32 query tokens, rounded, in A-fragment order in the workspace.
//   scan    a workgroup of four waves owns a GROUP of QG queries and 4 * bpw consecutive 32-row token blocks; it stages the QG * NAB
//           A blocks of its queries into LDS once, as they are packed.  Each wave owns bpw blocks and serves the docs that START
//           in them: it finds the first by a binary search of tok_ptr (wave-uniform; no host copy of tok_ptr) and runs past its
//           range's end to finish its last doc, so a doc longer than a range -- or than a workgroup's -- simply has one owner.  The
//           walk is doc-major over a cached block: the chains of block b (acc, QG * NAB sets of 16) are computed when a doc first
//           needs b and kept, so the doc that ends inside b and the docs that start inside b all fold the SAME accumulators, each
//           masked to its own columns, into the elementwise running max; a block's B fragments are loaded from the packed store
//           once per group, MS_G k-steps at a time (a wave's load of a k-step is a contiguous KiB), the next group -- of this block
//           or of the next one -- in flight over the QG * NAB * MS_G MFMAs of this one.  That reuse of a loaded fragment by
//           QG * NAB chains is the point of the kernel.  A chain is the reranker's: v_mfma_f32_32x32x16 over k ascending from
//           +0.0f, query tokens in A, doc tokens in B; a column of the result depends on its own B column only, so the rows of
//           neighbouring docs in the block change nothing.  The max is exact, so folding by store-aligned instead of doc-aligned
//           columns gives the same value (the sign of a zero max may differ; x + -0 and x + +0 are the same bits, and the sum
//           starts from +0.0f).  When a doc ends it is finished as the reranker does -- cross-lane max per half, readlane, ordered
//           sum over the live tokens -- and lane 0 writes the QG scores to the pass's f32[rows][ld] matrix.  A doc without tokens
//           gets +0.0f from the wave that owns the position it starts at (the last wave owns everything from its first row on,
//           the trailing empty docs included).
//           QG: the largest of 4, 2, 1 with QG * NAB <= 4 (32 accumulator + 32 running-max registers per set: 256 of the 512
//           a wave has at one wave per SIMD), QG * NAB * ks <= 64 (KiB of LDS) and QG < 2 nq (a lone query is not scanned four
//           times).  64 KiB rather than the 160 KiB a CU has: it is what a launch gets without opting in, and it only binds at
//           dim_pad >= 512, where a block already feeds >= 32 MFMAs per KiB loaded.  No top-k is fused into the scan: the matrix
//           costs 4 bytes per (query, doc) against some kilobytes of token rows.
//   select  64-bit keys (ms_order_key(score) : 0x7FFFFFFF - doc) -- the reranker's rank key, so negatives and +0.0f rank
//           correctly; 0 is "no doc" (a live key's low word is >= 1).  The selection helpers of srx_common.h key on the raw bits of
//           scores > 0 and are not used.  A workgroup folds its split of a score row in chunks into a sorted list in LDS: the
//           list (pow2ceil(k) keys) and the chunk share one 2048-key buffer; a chunk in which no allowed key beats the current
//           k-th is skipped, else the buffer is sorted (bitonic, descending).  The filter bit is read here.  With one split the
//           workgroup writes the query's row; else it stores its k keys and ...
//   merge   ... the same kernel, one workgroup per query, folds the splits' keys and writes doc / score / count and the padding.
#include "maxsim_common.h"
#include "late/sparse_rx_maxsim_search.h"

namespace {

constexpr int MS_G = 4;                  // k-steps per group of B loads, as in the reranker
constexpr int SS_LDS_KS = 64;            // QG * NAB * ks <= 64: a KiB of LDS per (A block, k-step)
constexpr int SS_MIN_BPW = 4;            // 32-row blocks per wave of the scan, at least
constexpr int SS_TARGET_WGS = 4096;      // workgroups the scan aims at
constexpr int SS_BUF = 2048;             // keys in the selection's LDS buffer: the list and a chunk
constexpr int64_t SS_SPLIT_DOCS = 8192;  // docs per split of a score row, at least
constexpr int SS_SPLIT_WGS = 2048;       // workgroups the selection aims at
constexpr int64_t SS_MATRIX_BYTES = 1ll << 30;

struct ScanArgs {
    const hf_v4i *tok;           // the packed token store: tiles * ks * 64 pieces
    const int32_t *tok_ptr;      // [n_docs + 1]
    const int32_t *q_tok_count;  // [nq] or null
    const hf_v4i *qpack;         // [nq][nab][ks][64]
    float *score;                // [rows][ld]
    int64_t n_tok, tiles, ld;
    int n_docs, q0, cnt, tq, ks, bpw, nranges;
};

struct SelArgs {
    const float *score;               // [rows][ld]
    const unsigned long long *keys_in;  // merge: [cnt][nsplit][k]
    unsigned long long *keys_out;     // select with nsplit > 1
    const uint32_t *fbits;            // null: no filter
    const int32_t *q_filter;
    int64_t fwords, ld, n_docs, doc_base, seg;
    int n_filters, q0, k, nsplit;
    int32_t *out_doc;
    float *out_score;
    int32_t *out_count;
};

// ================================================================================================ scan
template <int TYPE, int NAB, int QG>
__global__ __launch_bounds__(THREADS) void srx_maxsim_scan_kernel(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ss_smem[];
    hf_v4i *A = reinterpret_cast<hf_v4i *>(ss_smem);  // [QG][NAB][ks][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31;
    const int grp = (int)(blockIdx.x / (unsigned)a.nranges), range = (int)(blockIdx.x - (unsigned)grp * (unsigned)a.nranges);
    const int ks = a.ks, pieces = NAB * ks * 64, qbase = grp * QG;
    int live_t[QG];
#pragma unroll
    for (int qi = 0; qi < QG; ++qi) {
        const int q = a.q0 + min(qbase + qi, a.cnt - 1);  // past the pass: a copy of its last query, computed and not written
        const hf_v4i *qp = a.qpack + (int64_t)q * pieces;
        for (int i = tid; i < pieces; i += THREADS) A[qi * pieces + i] = qp[i];
        live_t[qi] = a.q_tok_count != nullptr ? min(max(gload_i32(a.q_tok_count + q), 0), a.tq) : a.tq;
    }
    __syncthreads();
    // the wave's rows [r0, r1): the first wave owns everything below r1, the last everything from r0 on
    const int w = range * WAVES + wave, nw = a.nranges * WAVES;
    const int64_t r0 = (int64_t)w * a.bpw * 32, r1 = r0 + (int64_t)a.bpw * 32;
    int lo = 0;
    if (w > 0) {  // the first doc with tok_ptr[d] >= r0
        int hi = a.n_docs;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if ((int64_t)uni(gload_i32(a.tok_ptr + mid)) < r0)
                lo = mid + 1;
            else
                hi = mid;
        }
    }
    const float NEG_INF = -__builtin_inff();
    const int gpb = ks / MS_G;
    float mx[QG * NAB][16];
    hf_v16f acc[QG * NAB];
#pragma unroll
    for (int j = 0; j < QG * NAB; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            mx[j][e] = NEG_INF;
            acc[j][e] = 0.0f;
        }
    hf_v4i pre[MS_G], cur[MS_G];
    int cb = -1, pre_blk = -1;  // the block whose chains acc holds; the block whose first group pre holds
    // k-steps s0 .. s0 + MS_G - 1 of block b (0 <= b < tiles): piece hf_piece(32 b + r, ks, s, h) = (b ks + s) 64 + lane
    auto load_group = [&](int b, int s0) __attribute__((always_inline)) {
        const hf_v4i *p = a.tok + ((int64_t)b * ks + s0) * 64 + lane;
#pragma unroll
        for (int u = 0; u < MS_G; ++u) pre[u] = p[u * 64];
    };
    for (int d = lo; d < a.n_docs; ++d) {  // uniform per wave
        const int s = uni(gload_i32(a.tok_ptr + d));
        if (w + 1 < nw && (int64_t)s >= r1) break;
        const int t0 = max(s, 0), t1 = uni((int)min((int64_t)gload_i32(a.tok_ptr + d + 1), a.n_tok));
        float score[QG];
#pragma unroll
        for (int qi = 0; qi < QG; ++qi) score[qi] = 0.0f;
        if (t1 > t0) {
            for (int b = t0 >> 5; b <= (t1 - 1) >> 5; ++b) {  // 0 <= b < tiles: t0 >= 0, t1 <= n_tok
                if (b != cb) {
                    if (pre_blk != b) load_group(b, 0);
#pragma unroll
                    for (int j = 0; j < QG * NAB; ++j)
#pragma unroll
                        for (int e = 0; e < 16; ++e) acc[j][e] = 0.0f;
                    for (int g = 0; g < gpb; ++g) {
#pragma unroll
                        for (int u = 0; u < MS_G; ++u) cur[u] = pre[u];
                        if (g + 1 < gpb) {  // in flight over this group's MFMAs
                            load_group(b, (g + 1) * MS_G);
                        } else if ((int64_t)b + 1 < a.tiles) {
                            load_group(b + 1, 0);
                            pre_blk = b + 1;
                        } else {
                            pre_blk = -1;
                        }
#pragma unroll
                        for (int u = 0; u < MS_G; ++u)  // ascending k: one chain per output element
#pragma unroll
                            for (int j = 0; j < QG * NAB; ++j) acc[j] = hf_mfma<TYPE>(A[(j * ks + g * MS_G + u) * 64 + lane], cur[u], acc[j]);
                    }
                    cb = b;
                }
                const int row = 32 * b + r;  // column r of the block is token row 32 b + r
                const bool in = row >= t0 && row < t1;
#pragma unroll
                for (int j = 0; j < QG * NAB; ++j)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const float v = acc[j][e];
                        mx[j][e] = (in && v > mx[j][e]) ? v : mx[j][e];
                    }
            }
            // the max over the 32 columns of each half; then row (e & 3) + 8 (e >> 2) + 4 h of block ab is in every lane of half h
#pragma unroll
            for (int j = 0; j < QG * NAB; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    float v = mx[j][e];
#pragma unroll
                    for (int o = 16; o > 0; o >>= 1) {
                        const float x = __shfl_xor(v, o);
                        v = x > v ? x : v;
                    }
                    mx[j][e] = v;
                }
            // the ordered sum: query token i = 32 ab + row, row = (e & 3) + 8 (e >> 2) + 4 h
#pragma unroll
            for (int qi = 0; qi < QG; ++qi)
#pragma unroll
                for (int ab = 0; ab < NAB; ++ab)
#pragma unroll
                    for (int row = 0; row < 32; ++row) {
                        const int e = (row & 3) + 4 * (row >> 3), hh = (row >> 2) & 1;
                        const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mx[qi * NAB + ab][e]), 32 * hh));
                        if (ab * 32 + row < live_t[qi]) score[qi] = score[qi] + v;
                    }
#pragma unroll
            for (int j = 0; j < QG * NAB; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) mx[j][e] = NEG_INF;
        }
        if (lane == 0) {
#pragma unroll
            for (int qi = 0; qi < QG; ++qi)
                if (qbase + qi < a.cnt) a.score[(int64_t)(qbase + qi) * a.ld + d] = score[qi];
        }
    }
}

// ================================================================================================ select / merge
template <bool MERGE>
__global__ __launch_bounds__(THREADS) void srx_maxsim_select_kernel(SelArgs a) {
    __shared__ unsigned long long buf[SS_BUF];  // [0, kl): the list, descending, zeros behind the live keys; [kl, 2048): the chunk
    __shared__ unsigned red[4 * WAVES];
    const int tid = threadIdx.x, k = a.k;
    const int ql = MERGE ? (int)blockIdx.x : (int)(blockIdx.x / (unsigned)a.nsplit);  // the query within the pass
    const int split = MERGE ? 0 : (int)(blockIdx.x - (unsigned)ql * (unsigned)a.nsplit);
    const int q = a.q0 + ql;
    int kl = 1;
    while (kl < k) kl <<= 1;  // <= 1024
    const int ch = SS_BUF - kl;
    int64_t begin, end;
    if (MERGE) {
        begin = 0;
        end = (int64_t)a.nsplit * k;
    } else {
        begin = (int64_t)split * a.seg;
        end = begin + a.seg < a.n_docs ? begin + a.seg : a.n_docs;
    }
    const uint32_t *frow = nullptr;  // the query's filter row
    bool none = false;               // a row number at or past n_filters: nothing is allowed, nothing outside the rows is read
    if (!MERGE && a.fbits != nullptr) {
        const int row = a.q_filter != nullptr ? gload_i32(a.q_filter + q) : 0;
        if (row >= a.n_filters)
            none = true;
        else if (row >= 0)
            frow = a.fbits + (int64_t)row * a.fwords;
    }
    for (int i = tid; i < kl; i += THREADS) buf[i] = 0ull;
    __syncthreads();
    for (int64_t c0 = begin; c0 < end; c0 += ch) {
        const unsigned long long thr = buf[k - 1];  // the k-th key of the list so far, 0 while it is not full
        int any = 0;
        for (int i = tid; i < ch; i += THREADS) {
            const int64_t idx = c0 + i;
            unsigned long long x = 0ull;
            if (idx < end) {
                if (MERGE) {
                    x = a.keys_in[(int64_t)ql * a.nsplit * k + idx];
                } else if (!none && (frow == nullptr || ((frow[idx >> 5] >> (idx & 31)) & 1u))) {
                    x = ((unsigned long long)ms_order_key(a.score[(int64_t)ql * a.ld + idx]) << 32) | (0x7FFFFFFFu - (unsigned)(a.doc_base + idx));
                }
            }
            if (x <= thr) x = 0ull;
            any |= x != 0ull;
            buf[kl + i] = x;
        }
        if (__syncthreads_or(any)) {  // else: nothing in the chunk beats the k-th key
            for (unsigned size = 2; size <= (unsigned)SS_BUF; size <<= 1) {
                for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
                    for (unsigned i = tid; i < (unsigned)(SS_BUF >> 1); i += THREADS) {
                        const unsigned pos = 2 * i - (i & (stride - 1));
                        const unsigned long long x = buf[pos], y = buf[pos + stride];
                        const bool desc = (pos & size) == 0;
                        if (desc ? (x < y) : (x > y)) {
                            buf[pos] = y;
                            buf[pos + stride] = x;
                        }
                    }
                    __syncthreads();
                }
            }
        }
    }
    if (!MERGE && a.nsplit > 1) {
        unsigned long long *out = a.keys_out + ((int64_t)ql * a.nsplit + split) * k;
        for (int i = tid; i < k; i += THREADS) out[i] = buf[i];
        return;
    }
    unsigned mine = 0;
    for (int i = tid; i < k; i += THREADS) mine += buf[i] != 0ull;
    const unsigned cnt = block_sum(mine, red);
    int32_t *od = a.out_doc + (int64_t)q * k;
    float *os = a.out_score + (int64_t)q * k;
    for (unsigned i = tid; i < (unsigned)k; i += THREADS) {
        if (i < cnt) {
            const unsigned long long x = buf[i];
            od[i] = (int32_t)(0x7FFFFFFFu - (unsigned)(x & 0xFFFFFFFFull));
            os[i] = ms_order_value((unsigned)(x >> 32));
        } else {
            od[i] = -1;
            os[i] = 0.0f;
        }
    }
    if (tid == 0) a.out_count[q] = (int)cnt;
}

// ================================================================================================ host side
// the query group of a call
inline int ss_group(int nab, int ks, int nq) {
    for (int g = 4; g > 1; g >>= 1)
        if (g * nab <= 4 && g * nab * ks <= SS_LDS_KS && g < 2 * nq) return g;
    return 1;
}
inline int ss_splits(int64_t n_docs, int rows) {
    const int64_t by_docs = (n_docs + SS_SPLIT_DOCS - 1) / SS_SPLIT_DOCS, cap = SS_SPLIT_WGS / rows > 1 ? SS_SPLIT_WGS / rows : 1;
    return (int)(by_docs < cap ? by_docs : cap);
}
struct SearchPlan {
    int qg, rows, splits;  // queries per group; score rows and splits per row of the preferred pass
    int64_t ld, qbytes, min_bytes, bytes;
};
inline SearchPlan ss_plan(int nq, int tq, int dim_pad, int64_t n_docs, int k) {
    SearchPlan p;
    p.qg = ss_group(ceil32(tq) / 32, dim_pad / 16, nq);
    p.ld = (n_docs + 63) / 64 * 64;
    int64_t pass = SS_MATRIX_BYTES / (p.ld * 4) / 4 * 4;
    pass = pass < 4 ? 4 : pass > 1024 ? 1024 : pass;
    p.rows = (int)(nq < pass ? nq : pass);
    p.splits = p.rows > 0 ? ss_splits(n_docs, p.rows) : 1;
    p.qbytes = qpack_bytes(nq, tq, dim_pad);
    p.min_bytes = p.qbytes + (int64_t)(nq < p.qg ? nq : p.qg) * p.ld * 4 + 512;
    p.bytes = p.qbytes + p.rows * p.ld * 4 + (p.splits > 1 ? ((int64_t)p.rows * p.splits * k * 8 + 255) / 256 * 256 : 0) + 512;
    return p;
}

template <int TYPE>
void launch_scan(const ScanArgs &a, int nab, int qg, hipStream_t stream) {
    const dim3 grid((unsigned)((int64_t)a.nranges * ((a.cnt + qg - 1) / qg)));  // <= SS_TARGET_WGS + groups + 1
    const size_t lds = (size_t)qg * nab * a.ks * 64 * 16;                         // <= 64 KiB
#define SRX_SS(NAB, QG)                                                                                         \
    if (nab == NAB && qg == QG) {                                                                               \
        hipLaunchKernelGGL((srx_maxsim_scan_kernel<TYPE, NAB, QG>), grid, dim3(THREADS), lds, stream, a);       \
        return;                                                                                                 \
    }
    SRX_SS(1, 4) SRX_SS(1, 2) SRX_SS(1, 1) SRX_SS(2, 2) SRX_SS(2, 1) SRX_SS(3, 1) SRX_SS(4, 1)
#undef SRX_SS
}

bool dims_ok(int32_t nq, int32_t tq, int32_t dim_pad, int64_t n_docs, int32_t k) {
    return nq >= 0 && hf_dim_ok(dim_pad) && tq_ok(tq, dim_pad) && n_docs >= 1 && n_docs <= SRX_FILTER_MAX_DOCS && k >= 1 && k <= KMAX;
}

}  // namespace

SRX_API int64_t srx_maxsim_search_workspace_bytes(int32_t nq, int32_t tq, int32_t dim_pad, int64_t n_docs, int32_t k) {
    if (!dims_ok(nq, tq, dim_pad, n_docs, k))
        return fail(SRX_ERR_INVALID, "srx_maxsim_search_workspace_bytes: need nq >= 0, tq in 1 .. 128 with ceil32(tq) * dim_pad <= 32768, "
                                     "n_docs in [1, 2^31 - 2], k in 1 .. 1024%s");
    return ss_plan(nq, tq, dim_pad, n_docs, k).bytes;
}

SRX_API int srx_maxsim_search_half(int32_t device, int32_t type, const void *tok_packed, int64_t n_tok, int32_t dim_pad,
                                   const int32_t *tok_ptr, int64_t n_docs, int64_t doc_base, const float *q_tok, const int32_t *q_tok_count,
                                   int32_t nq, int32_t tq, int32_t k, const srx_doc_filter *filter, int32_t *out_doc, float *out_score,
                                   int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream_v) {
    const char *who = "srx_maxsim_search_half";
    if (type != SRX_HALF_F16 && type != SRX_HALF_BF16) return fail(SRX_ERR_INVALID, "%s: type must be SRX_HALF_F16 or SRX_HALF_BF16", who);
    if (!hf_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 64, <= 1024 (pad the rows with zeros)", who);
    if (!tq_ok(tq, dim_pad)) return fail(SRX_ERR_INVALID, "%s: tq must be in 1 .. 128 with ceil32(tq) * dim_pad <= 32768", who);
    if (k < 1 || k > KMAX) return fail(SRX_ERR_INVALID, "%s: k must be in 1 .. 1024", who);
    if (n_docs <= 0 || n_docs > SRX_FILTER_MAX_DOCS) return fail(SRX_ERR_INVALID, "%s: n_docs out of range", who);
    if (n_tok < 0 || n_tok >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: n_tok out of range", who);
    if (doc_base < 0 || doc_base + n_docs > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: doc_base < 0 or doc_base + n_docs > 2^31 - 1", who);
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if (filter != nullptr) {
        const int rc = srx_check_filter(who, filter);
        if (rc != SRX_OK) return rc;
    }
    if (nq == 0) return SRX_OK;
    if (!tok_ptr || !q_tok || !out_doc || !out_score || !out_count || (n_tok > 0 && !tok_packed)) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)tok_packed | (uintptr_t)q_tok) & 15) return fail(SRX_ERR_INVALID, "%s: tok_packed / q_tok must be 16-byte aligned", who);
    const SearchPlan pl = ss_plan(nq, tq, dim_pad, n_docs, k);
    if (!workspace || workspace_bytes < pl.min_bytes) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    // the pass of THIS workspace: as many score rows as fit, whole groups when there are several passes; the key lists in the rest
    const int64_t row_bytes = pl.ld * 4, avail = workspace_bytes - 512 - pl.qbytes;
    int rows = (int)(avail / row_bytes < pl.rows ? avail / row_bytes : pl.rows);
    if (rows < nq && rows > pl.qg) rows = rows / pl.qg * pl.qg;
    int nsplit = ss_splits(n_docs, rows);
    const int64_t lists = (avail - rows * row_bytes) / ((int64_t)rows * k * 8);
    if (nsplit > lists) nsplit = (int)lists;
    if (nsplit < 2) nsplit = 1;
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    char *base = (char *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    const int nab = ceil32(tq) / 32, ks = dim_pad / 16;
    MaxsimArgs pk = {};
    pk.q_tok = q_tok;
    pk.qpack = (hf_v4i *)base;
    pk.nq = nq;
    pk.tq = tq;
    pk.nab = nab;
    pk.ks = ks;
    const int64_t pack_pieces = (int64_t)nq * nab * ks * 64, pack_blocks = (pack_pieces + THREADS - 1) / THREADS;
    const dim3 pack_grid((unsigned)(pack_blocks < 65536 ? pack_blocks : 65536));
    if (type == SRX_HALF_F16)
        hipLaunchKernelGGL(srx_maxsim_pack_kernel<SRX_HALF_F16>, pack_grid, dim3(THREADS), 0, stream, pk);
    else
        hipLaunchKernelGGL(srx_maxsim_pack_kernel<SRX_HALF_BF16>, pack_grid, dim3(THREADS), 0, stream, pk);
    HIP_TRY(hipGetLastError());
    ScanArgs sa = {};
    sa.tok = (const hf_v4i *)tok_packed;
    sa.tok_ptr = tok_ptr;
    sa.q_tok_count = q_tok_count;
    sa.qpack = (const hf_v4i *)base;
    sa.score = (float *)(base + pl.qbytes);
    sa.n_tok = n_tok;
    sa.tiles = hf_tiles(n_tok);
    sa.ld = pl.ld;
    sa.n_docs = (int)n_docs;
    sa.tq = tq;
    sa.ks = ks;
    SelArgs se = {};
    se.score = sa.score;
    se.keys_out = (unsigned long long *)(base + pl.qbytes + rows * row_bytes);
    se.keys_in = se.keys_out;
    if (filter != nullptr) {
        se.fbits = filter->bits;
        se.q_filter = filter->q_filter;
        se.n_filters = filter->n_filters;
        se.fwords = srx_filter_row_words(n_docs);
    }
    se.ld = pl.ld;
    se.n_docs = n_docs;
    se.doc_base = doc_base;
    se.seg = (n_docs + nsplit - 1) / nsplit;
    se.k = k;
    se.nsplit = nsplit;
    se.out_doc = out_doc;
    se.out_score = out_score;
    se.out_count = out_count;
    for (int q0 = 0; q0 < nq; q0 += rows) {
        const int cnt = nq - q0 < rows ? nq - q0 : rows, groups = (cnt + pl.qg - 1) / pl.qg;
        const int64_t per_group = SS_TARGET_WGS / groups > 1 ? SS_TARGET_WGS / groups : 1;
        int64_t bpw = (sa.tiles + WAVES * per_group - 1) / (WAVES * per_group);
        if (bpw < SS_MIN_BPW) bpw = SS_MIN_BPW;
        const int64_t nranges = (sa.tiles + WAVES * bpw - 1) / (WAVES * bpw);
        sa.q0 = se.q0 = q0;
        sa.cnt = cnt;
        sa.bpw = (int)bpw;
        sa.nranges = (int)(nranges < 1 ? 1 : nranges);
        if (type == SRX_HALF_F16)
            launch_scan<SRX_HALF_F16>(sa, nab, pl.qg, stream);
        else
            launch_scan<SRX_HALF_BF16>(sa, nab, pl.qg, stream);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(srx_maxsim_select_kernel<false>, dim3((unsigned)(cnt * nsplit)), dim3(THREADS), 0, stream, se);
        HIP_TRY(hipGetLastError());
        if (nsplit > 1) {
            hipLaunchKernelGGL(srx_maxsim_select_kernel<true>, dim3((unsigned)cnt), dim3(THREADS), 0, stream, se);
            HIP_TRY(hipGetLastError());
        }
    }
    return SRX_OK;
}
