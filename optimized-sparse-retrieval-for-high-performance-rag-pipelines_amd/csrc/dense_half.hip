// dense_half.hip -- the half-precision dense index (include/sparse_rx_half.h): f16 / bf16 rows in MFMA-fragment order, the
// conversion that writes them, a batched GEMM search and the scorer of given docs.  Replaces nothing in the reference
// project: it has no half-precision index.
//
// A translation unit of its own (as filter.hip is): it is a second user of topk_fold / topk_shrink, and inside dense.hip
// or filter.hip that would change what the compiler inlines into the kernels already there.
//
//   convert   one workgroup per tile of 32 rows, one wave per row at a time: the row is read once (16-byte loads when the
//             base, ld and dim allow), rounded in registers, a non-finite row found by a ballot and zeroed; the 16-bit codes
//             go to the tile's image in LDS and leave it in fragment order, a contiguous KiB per (tile, k-step).
//   pack      the f32 query block of a pass, rounded, in the same order (tiles past the batch are zeros).
//   GEMM      a workgroup = 128 queries x 128 docs, four waves as 2 x 2, a wave = 2 x 2 tiles of 32 x 32.  The K loop moves
//             HG_KB k-steps (64 columns) per stage: both operands' fragment-ordered KiBs are staged through LDS as they are
//             (a wave's ds_read_b128 of a fragment is a contiguous KiB: no bank conflicts), two buffers, the next stage's
//             global loads in flight over the MFMAs of this one, one barrier per stage.  Every output element is ONE chain of
//             the instruction over s = 0, 1, ... in ascending order from +0.0f.  The scores go to a [queries][ld] fp32 matrix.
//   rank      srx_filtered_topk_kernel's fold loop with the filter row optional and the offset applied, then srx_merge_impl.
//   scorer    one wave per (query, 32 candidates): the candidates' pieces gathered as the B operand, the query in every row
//             of A, the same chain; row 0 of the result is read.
#include "half_common.h"

namespace {

constexpr int HG_KB = 4;  // k-steps per stage of the GEMM's K loop (dim_pad is a multiple of 64 = 4 k-steps)
static_assert(THREADS == HG_KB * 64, "the GEMM's staging moves piece threadIdx.x of each tile's HG_KB KiB: one piece per thread");
static_assert(WAVES == 4 && HF_QTILE == 128, "the GEMM lays its four waves out 2 x 2 over 128 queries x 128 docs");

// ================================================================================================ convert
constexpr int HC_TILE = 32;               // rows per workgroup
constexpr int HC_ROWS = HC_TILE / WAVES;  // rows per wave
static_assert(HC_TILE % WAVES == 0, "the convert kernel gives every wave the same number of rows of a tile");

struct HalfConvertArgs {
    const float *in;        // the chunk's rows (row stride ld elements)
    int64_t ld, n_rows;     // rows of this call
    int64_t row0;           // where they sit in the whole corpus
    int dim, dim_pad;
    hf_v4i *out;            // the WHOLE corpus in fragment order
    int32_t *flag;          // may be null
};

template <int NJ, bool VEC, int TYPE>
__global__ __launch_bounds__(THREADS) void srx_dense_half_convert_kernel(HalfConvertArgs a) {
    constexpr int PITCH = NJ * 512 + 16;  // bytes between two rows of the tile image (16-byte reads down a column of 32 rows: different banks)
    __shared__ __attribute__((aligned(16))) unsigned char tile[HC_TILE * PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * HC_TILE;            // the tile's first row, relative to row0
    const int live = (int)min((int64_t)HC_TILE, a.n_rows - t0);  // rows of the tile this call holds (>= 1)
    bool flagged = false;                                        // wave-uniform
    for (int g = 0; g < HC_ROWS; ++g) {
        const int r = wave * HC_ROWS + g;
        uint2 *trow = reinterpret_cast<uint2 *>(tile + r * PITCH);
        const float *row = a.in + (t0 + r) * a.ld;
        unsigned code[NJ][4];
        bool bad = false;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = 4 * lane + 256 * j;
            float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // columns past dim and rows the call does not hold: zeros
            if (r < live) {
                if constexpr (VEC) {  // dim % 4 == 0: the four columns are inside the row together
                    if (c < a.dim) {
                        const hf_v4f v = *reinterpret_cast<const hf_v4f *>(row + c);
                        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < a.dim) x[e] = row[c + e];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) code[j][e] = hf_round<TYPE>(x[e], bad);
        }
        bad = __ballot(bad) != 0ull;  // the whole row is the wave's
        flagged = flagged || bad;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int c = 4 * lane + 256 * j;
            if (c < a.dim_pad) trow[lane + 64 * j] = bad ? make_uint2(0u, 0u) : make_uint2(code[j][0] | (code[j][1] << 16), code[j][2] | (code[j][3] << 16));
        }
    }
    if (flagged && lane == 0 && a.flag != nullptr) atomicOr(a.flag, SRX_QUANT_NONFINITE);
    __syncthreads();
    // piece i of the tile: k-step i >> 6, lane i & 63 = row (i & 31), half (i >> 5) & 1
    const int pieces = 4 * a.dim_pad;  // dim_pad / 16 k-steps of 64
    const int64_t base = ((a.row0 >> 5) + blockIdx.x) * (int64_t)pieces;
    for (int i = threadIdx.x; i < pieces; i += THREADS) {
        const int ln = i & 63;
        a.out[base + i] = *reinterpret_cast<const hf_v4i *>(tile + (ln & 31) * PITCH + 32 * (i >> 6) + 16 * (ln >> 5));
    }
}

template <int TYPE>
void hc_launch(const HalfConvertArgs &a, bool vec, hipStream_t stream) {
    const unsigned blocks = (unsigned)((a.n_rows + HC_TILE - 1) / HC_TILE);
    const int nj = (a.dim_pad + 255) / 256;
#define SRX_HC(NJ)                                                                                                                  \
    if (nj == NJ) {                                                                                                                 \
        if (vec)                                                                                                                    \
            hipLaunchKernelGGL((srx_dense_half_convert_kernel<NJ, true, TYPE>), dim3(blocks), dim3(THREADS), 0, stream, a);         \
        else                                                                                                                        \
            hipLaunchKernelGGL((srx_dense_half_convert_kernel<NJ, false, TYPE>), dim3(blocks), dim3(THREADS), 0, stream, a);        \
        return;                                                                                                                     \
    }
    SRX_HC(1) SRX_HC(2) SRX_HC(3) SRX_HC(4)
#undef SRX_HC
}

// ================================================================================================ query pack
// qpack[(tile * ks + s) * 64 + lane] = the rounded columns 16 s + 8 (lane >> 5) .. + 7 of query tile * 32 + (lane & 31);
// n_tiles tiles are written, queries at or past nq as zeros
template <int TYPE>
__global__ __launch_bounds__(THREADS) void srx_dense_half_pack_queries_kernel(const float *__restrict__ queries, int nq, int ks, int n_tiles,
                                                                              hf_v4i *__restrict__ qpack) {
    const int64_t n = (int64_t)n_tiles * ks * 64;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const int lane = (int)(i & 63);
        const int64_t ts = i >> 6;
        const int s = (int)(ts % ks);
        const int64_t q = (ts / ks) * 32 + (lane & 31);
        hf_v4i p = {0, 0, 0, 0};
        if (q < nq) {
            const hf_v4f *src = reinterpret_cast<const hf_v4f *>(queries + q * (int64_t)(ks * 16) + 16 * s + 8 * (lane >> 5));
            p = hf_round8<TYPE>(src[0], src[1]);
        }
        qpack[i] = p;
    }
}

// ================================================================================================ GEMM
// D[row = query][col = doc]: lane l holds doc l & 31, rows (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).  Workgroup b serves query
// block b % n_qblocks and doc block b / n_qblocks: the workgroups that read one block of docs run together.
template <int TYPE>
__global__ __launch_bounds__(THREADS) void srx_dense_half_scores_kernel(const hf_v4i *__restrict__ corpus, int64_t n_docs, int ks,
                                                                        const hf_v4i *__restrict__ qpack, int nq, int n_qblocks,
                                                                        float *__restrict__ scores, int64_t ld) {
    __shared__ hf_v4i stage[2][2][4][HG_KB * 64];  // [buffer][queries / docs][tile of 32][k-step of the stage][lane]: 64 KiB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int qblock = (int)(blockIdx.x % (unsigned)n_qblocks);
    const int64_t dblock = blockIdx.x / (unsigned)n_qblocks;
    const int64_t qt0 = (int64_t)qblock * 4, dt0 = dblock * 4;  // first tiles of 32; the query tiles all exist in qpack
    const int64_t n_dtiles = (n_docs + 31) / 32;                // tiles the corpus holds: nothing is read past them
    const int wq = wave >> 1, wd = wave & 1;                    // the wave's 64 queries and 64 docs of the block
    hf_v4i ga[4], gb[4];
    // thread t moves piece t of each tile's HG_KB KiB of the stage: (tile * ks + s0) * 64 + t, t < HG_KB * 64 = 256
    auto load_stage = [&](int st) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ga[i] = qpack[((qt0 + i) * ks + st * HG_KB) * 64 + tid];
            gb[i] = (hf_v4i){0, 0, 0, 0};
            if (dt0 + i < n_dtiles) gb[i] = corpus[((dt0 + i) * ks + st * HG_KB) * 64 + tid];
        }
    };
    auto store_stage = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            stage[buf][0][i][tid] = ga[i];
            stage[buf][1][i][tid] = gb[i];
        }
    };
    hf_v16f acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.0f;
    const int n_stages = ks / HG_KB;
    load_stage(0);
    store_stage(0);
    __syncthreads();
    for (int st = 0; st < n_stages; ++st) {
        const int buf = st & 1;
        const bool more = st + 1 < n_stages;  // uniform
        if (more) load_stage(st + 1);         // in flight over this stage's MFMAs
#pragma unroll
        for (int kk = 0; kk < HG_KB; ++kk) {  // ascending k: one chain per output element
            hf_v4i A[2], B[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                A[i] = stage[buf][0][2 * wq + i][kk * 64 + lane];
                B[i] = stage[buf][1][2 * wd + i][kk * 64 + lane];
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = hf_mfma<TYPE>(A[i], B[j], acc[i][j]);
        }
        if (more) store_stage(buf ^ 1);  // that buffer was last read in stage st - 1: one barrier ago
        __syncthreads();
    }
    const int64_t q0 = (qt0 + 2 * wq) * 32, d0 = (dt0 + 2 * wd) * 32;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t d = d0 + 32 * j + r;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int64_t q = q0 + 32 * i + (reg & 3) + 8 * (reg >> 2) + 4 * h;
                if (q < nq && d < n_docs) scores[q * ld + d] = acc[i][j][reg];
            }
        }
}

// ================================================================================================ rank
// One workgroup per (query, split of the columns) folds its slice of the score row into an exact lazy top-k list: the ranked
// value of column c is fl32(score + offset), a result iff > 0 and (with a filter row) bit c of the row is set.
__global__ __launch_bounds__(THREADS) void srx_dense_half_topk_kernel(const float *__restrict__ scores, int64_t ld, int64_t n_docs, int nq,
                                                                      int k, int n_splits, int64_t doc_base, float score_offset,
                                                                      const uint32_t *__restrict__ filter_bits, int64_t filter_words,
                                                                      const int32_t *__restrict__ q_filter, int q0,
                                                                      int32_t *__restrict__ cand_doc, float *__restrict__ cand_score,
                                                                      int32_t *__restrict__ cand_count) {
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
constexpr int HS_CHUNK = 32;  // candidates per wave: the columns of one MFMA tile
struct HalfScoreArgs {
    const hf_v4i *corpus;
    const float *queries;
    const int32_t *cand_doc, *cand_count;
    float *out_score;
    int64_t n_docs, doc_base, waves;  // waves = nq * chunks
    int ks, m, chunks;
};
template <int TYPE>
__global__ __launch_bounds__(THREADS) void srx_dense_half_score_docs_kernel(HalfScoreArgs a) {
    const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
    const int64_t w = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (w >= a.waves) return;  // whole waves leave
    const int q = (int)(w / a.chunks);
    const int64_t c = (w - (int64_t)q * a.chunks) * HS_CHUNK + r;  // both halves of the wave hold candidate r's row; 64 bits: the
    int64_t lim = a.m;                                             // last chunk of an m near 2^31 ends past int
    if (a.cand_count != nullptr) lim = min(lim, (int64_t)max(gload_i32(a.cand_count + q), 0));
    int row = -1;  // padding, outside the corpus, beyond m
    if (c < lim) {
        const int64_t local = (int64_t)gload_i32(a.cand_doc + (int64_t)q * a.m + c) - a.doc_base;
        if (local >= 0 && local < a.n_docs) row = (int)local;  // n_docs < 2^31
    }
    float res = 0.0f;
    if (__ballot(row >= 0) != 0ull) {  // uniform
        const hf_v4f *qrow = reinterpret_cast<const hf_v4f *>(a.queries + (int64_t)q * (a.ks * 16) + 8 * h);
        const hf_v4i *prow = a.corpus + hf_piece(row >= 0 ? row : 0, a.ks, 0, h);  // + 64 per k-step
        hf_v16f acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
        for (int s0 = 0; s0 < a.ks; s0 += 4) {  // the search's chain: ascending k from +0.0f; the query is every row of A
            hf_v4i A[4], B[4];                 // ks is a multiple of 4: four gathers in flight
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                B[u] = (hf_v4i){0, 0, 0, 0};
                if (row >= 0) B[u] = prow[(int64_t)(s0 + u) * 64];
                A[u] = hf_round8<TYPE>(qrow[4 * (s0 + u)], qrow[4 * (s0 + u) + 1]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = hf_mfma<TYPE>(A[u], B[u], acc);
        }
        if (row >= 0) res = acc[0];  // lanes 0 .. 31, register 0: row 0 of the tile, column = candidate r
    }
    if (h == 0 && c < a.m) a.out_score[(int64_t)q * a.m + c] = res;
}

// ================================================================================================ host side
bool type_ok(int32_t type) { return type == SRX_HALF_F16 || type == SRX_HALF_BF16; }

}  // namespace

SRX_API int64_t srx_dense_half_bytes(int64_t n_rows, int32_t dim_pad) {
    if (n_rows < 0 || !hf_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "srx_dense_half_bytes: need n_rows >= 0 and dim_pad a multiple of 64, <= 1024%s");
    return hf_tiles(n_rows) * 32 * (int64_t)dim_pad * 2;
}

SRX_API int srx_dense_convert_half(int32_t device, int32_t type, const float *emb, int64_t ld, int64_t n_rows, int32_t dim, int32_t dim_pad,
                                   int64_t row0, int64_t n_total, void *out_packed, int32_t *flag, void *stream_v) {
    const char *who = "srx_dense_convert_half";
    if (!type_ok(type)) return fail(SRX_ERR_INVALID, "%s: type must be SRX_HALF_F16 or SRX_HALF_BF16", who);
    if (n_rows < 0 || row0 < 0 || n_total < 0) return fail(SRX_ERR_INVALID, "%s: negative count", who);
    if (row0 > n_total || n_rows > n_total - row0) return fail(SRX_ERR_INVALID, "%s: row0 + n_rows > n_total", who);
    if (!hf_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: unsupported dim_pad (a multiple of 64, <= 1024)", who);
    if (dim < 1 || dim > dim_pad || ld < dim) return fail(SRX_ERR_INVALID, "%s: need 1 <= dim <= dim_pad and ld >= dim", who);
    if ((row0 & 31) != 0) return fail(SRX_ERR_INVALID, "%s: row0 must be a multiple of 32", who);
    if ((n_rows + HC_TILE - 1) / HC_TILE > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: too many rows in one call", who);
    if (n_rows == 0) return SRX_OK;
    if (!emb || !out_packed) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)emb & 3) return fail(SRX_ERR_INVALID, "%s: input must be 4-byte aligned", who);
    if ((uintptr_t)out_packed & 15) return fail(SRX_ERR_INVALID, "%s: out_packed must be 16-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    const HalfConvertArgs a = {emb, ld, n_rows, row0, dim, dim_pad, (hf_v4i *)out_packed, flag};
    const bool vec = ((uintptr_t)emb & 15) == 0 && ld % 4 == 0 && dim % 4 == 0;
    if (type == SRX_HALF_F16)
        hc_launch<SRX_HALF_F16>(a, vec, (hipStream_t)stream_v);
    else
        hc_launch<SRX_HALF_BF16>(a, vec, (hipStream_t)stream_v);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int64_t srx_dense_half_workspace_bytes(int32_t nq, int64_t n_docs, int32_t k) {
    if (nq < 0 || n_docs <= 0 || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "srx_dense_half_workspace_bytes: bad argument%s");
    return half_ws(nullptr, half_plan(nq, n_docs, k), k).bytes;
}

SRX_API int srx_dense_search_half(int32_t device, int32_t type, const void *corpus_packed, int64_t n_docs, int32_t dim_pad,
                                  const float *queries, int32_t nq, int32_t k, int64_t doc_base, const srx_doc_filter *filter,
                                  int32_t *out_doc, float *out_score, int32_t *out_count, void *workspace, int64_t workspace_bytes,
                                  void *stream_v, float score_offset) {
    const char *who = "srx_dense_search_half";
    if (!type_ok(type)) return fail(SRX_ERR_INVALID, "%s: type must be SRX_HALF_F16 or SRX_HALF_BF16", who);
    if (filter != nullptr) {
        const int rc = srx_check_filter(who, filter);
        if (rc != SRX_OK) return rc;
    }
    if (nq < 0 || n_docs <= 0 || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "%s: need n_docs > 0, 1 <= k <= 1024", who);
    if (!hf_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 64, <= 1024 (pad the rows with zeros)", who);
    if (doc_base < 0 || doc_base + n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: doc_base + n_docs must fit int32", who);
    if (nq == 0) return SRX_OK;
    if (!corpus_packed || !queries || !out_doc || !out_score || !out_count) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)corpus_packed | (uintptr_t)queries) & 15) return fail(SRX_ERR_INVALID, "%s: corpus / queries must be 16-byte aligned", who);
    const HalfPlan p = half_plan(nq, n_docs, k);
    const HalfWs w = half_ws(workspace, p, k);
    if (!workspace || workspace_bytes < w.bytes) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    const int ks = dim_pad / 16;
    const int64_t n_dblocks = (n_docs + HF_QTILE - 1) / HF_QTILE;
    const uint32_t *fbits = filter ? filter->bits : nullptr;
    const int32_t *qf = filter ? filter->q_filter : nullptr;
    for (int q0 = 0; q0 < nq; q0 += p.QB) {
        const int qb = nq - q0 < p.QB ? nq - q0 : p.QB;
        const int n_qblocks = (qb + HF_QTILE - 1) / HF_QTILE;
        const float *qsrc = queries + (int64_t)q0 * dim_pad;
        const unsigned pack_grid = (unsigned)(((int64_t)n_qblocks * 4 * ks * 64 + THREADS - 1) / THREADS);
        const dim3 grid((unsigned)(n_dblocks * n_qblocks));  // <= 2^24 * 8
        if (type == SRX_HALF_F16) {
            hipLaunchKernelGGL(srx_dense_half_pack_queries_kernel<SRX_HALF_F16>, dim3(pack_grid), dim3(THREADS), 0, stream, qsrc, qb, ks, n_qblocks * 4, w.qpack);
            hipLaunchKernelGGL(srx_dense_half_scores_kernel<SRX_HALF_F16>, grid, dim3(THREADS), 0, stream, (const hf_v4i *)corpus_packed, n_docs, ks,
                               (const hf_v4i *)w.qpack, qb, n_qblocks, w.scores, p.ld);
        } else {
            hipLaunchKernelGGL(srx_dense_half_pack_queries_kernel<SRX_HALF_BF16>, dim3(pack_grid), dim3(THREADS), 0, stream, qsrc, qb, ks, n_qblocks * 4, w.qpack);
            hipLaunchKernelGGL(srx_dense_half_scores_kernel<SRX_HALF_BF16>, grid, dim3(THREADS), 0, stream, (const hf_v4i *)corpus_packed, n_docs, ks,
                               (const hf_v4i *)w.qpack, qb, n_qblocks, w.scores, p.ld);
        }
        hipLaunchKernelGGL(srx_dense_half_topk_kernel, dim3((unsigned)((int64_t)qb * p.ns)), dim3(THREADS), 0, stream, (const float *)w.scores, p.ld, n_docs,
                           qb, (int)k, p.ns, doc_base, score_offset, fbits, srx_filter_row_words(n_docs), qf, q0, w.cand.doc, w.cand.score, w.cand.count);
        HIP_TRY(hipGetLastError());
        const srx_rows out = srx_plain_rows(out_doc + (int64_t)q0 * k, out_score + (int64_t)q0 * k, out_count + q0, k);
        const int rc = srx_merge_impl(device, w.cand, qb, p.ns, k, 0, out, nullptr, 0, stream_v);
        if (rc != SRX_OK) return rc;
    }
    return SRX_OK;
}

SRX_API int srx_dense_score_docs_half(int32_t device, int32_t type, const void *corpus_packed, int64_t n_docs, int32_t dim_pad,
                                      const float *queries, int32_t nq, int64_t doc_base, const int32_t *cand_doc, const int32_t *cand_count,
                                      int32_t m, float *out_score, void *stream_v) {
    const char *who = "srx_dense_score_docs_half";
    if (!type_ok(type)) return fail(SRX_ERR_INVALID, "%s: type must be SRX_HALF_F16 or SRX_HALF_BF16", who);
    if (!hf_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 64, <= 1024 (pad the rows with zeros)", who);
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if (m < 1) return fail(SRX_ERR_INVALID, "%s: m must be >= 1", who);
    if ((int64_t)nq * (int64_t)m > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: nq * m must fit int32", who);
    if (n_docs <= 0 || n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: n_docs out of range", who);
    if (doc_base < 0) return fail(SRX_ERR_INVALID, "%s: doc_base < 0", who);
    if (nq == 0) return SRX_OK;
    if (!corpus_packed || !queries || !cand_doc || !out_score) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)corpus_packed | (uintptr_t)queries) & 15) return fail(SRX_ERR_INVALID, "%s: corpus / queries must be 16-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    const int chunks = (int)(((int64_t)m + HS_CHUNK - 1) / HS_CHUNK);
    const HalfScoreArgs a = {(const hf_v4i *)corpus_packed, queries, cand_doc, cand_count, out_score, n_docs, doc_base, (int64_t)nq * chunks, dim_pad / 16, m, chunks};
    const dim3 grid((unsigned)((a.waves + WAVES - 1) / WAVES));  // waves <= nq * m < 2^31
    if (type == SRX_HALF_F16)
        hipLaunchKernelGGL(srx_dense_half_score_docs_kernel<SRX_HALF_F16>, grid, dim3(THREADS), 0, (hipStream_t)stream_v, a);
    else
        hipLaunchKernelGGL(srx_dense_half_score_docs_kernel<SRX_HALF_BF16>, grid, dim3(THREADS), 0, (hipStream_t)stream_v, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
