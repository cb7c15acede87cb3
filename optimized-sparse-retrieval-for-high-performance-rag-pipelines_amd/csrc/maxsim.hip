// maxsim.hip -- late-interaction reranking (include/sparse_rx_maxsim.h): MaxSim scores of given (query, doc) pairs over the
// token rows of a packed half corpus, and the top-k of a candidate list by them.  Replaces nothing in the reference project:
// it has no reranker and no multi-vector index.  Same build flags as the other units; -ffp-contract=off is part of the
// contract (every add of the ordered sum is rounded on its own).
//
// Up to three launches per call:
//   pack    the call's f32 query tokens, rounded to the corpus type, in A-fragment order in the workspace: per query
//           ceil32(tq) / 32 blocks of 32 tokens, a KiB per (block, k-step); tokens at or past tq are zero rows.
//   score   a workgroup of four waves serves one query and a slice of MS_SLICE candidates.  It stages the query's A fragments
//           into LDS once, as they are packed (a wave's ds_read_b128 of a fragment is a contiguous KiB: no bank conflicts).  A
//           wave takes whole candidate docs.  Per block of 32 doc tokens it loads the B fragments straight from the packed
//           store -- lane (r, h) reads piece hf_piece(t0 + 32 b + r, ks, s, h); consecutive token rows are consecutive
//           16-byte pieces inside a tile -- MS_G k-steps at a time, the next group in flight over the MFMAs of this one, and
//           runs ONE chain of v_mfma_f32_32x32x16 per A block, k ascending from +0.0f: the chain of
//           srx_dense_score_docs_half with 32 query tokens in A where that scorer repeats its query.  Token rows past the
//           doc's range are loaded as zeros AND masked out of the max (a lane's column is one doc token).  The running max is
//           kept elementwise in registers across the doc's blocks; only at the end of the doc is it reduced across the 32
//           lanes of each half, and the live query tokens are summed in ascending order.
//   rank    (rerank form) one workgroup per query: a bitonic sort of (order-preserving score key : 0x7FFFFFFF - doc) over
//           the live positions.  The selection helpers of srx_common.h key on the raw bits of scores > 0; MaxSim scores may
//           be negative, so the key maps the fp32 total order to unsigned order instead.
#include "half_common.h"
#include "sparse_rx_maxsim.h"

namespace {

constexpr int MS_SLICE = 32;         // candidates per workgroup of the score kernel
constexpr int MS_G = 4;              // k-steps per group of B loads (dim_pad is a multiple of 64 = 4 k-steps)
constexpr int MS_LDS_MAX = 64 << 10; // the A fragments of one query: ceil32(tq) * dim_pad * 2 bytes

struct MaxsimArgs {
    const hf_v4i *tok;        // the packed token store
    const int32_t *tok_ptr;   // [n_docs + 1]
    const float *q_tok;       // [nq][tq][dim_pad]
    const int32_t *q_tok_count;  // may be null
    const int32_t *cand_doc, *cand_count;  // cand_count may be null
    hf_v4i *qpack;            // [nq][nab][ks][64]
    float *score;             // [nq][m]: out_score of the scorer form, the workspace matrix of the rerank form
    int32_t *out_doc;         // rerank form
    float *out_score;
    int32_t *out_count;
    int64_t n_tok, n_docs, doc_base;
    int nq, tq, nab, ks, m, k, slices;
};

inline int ceil32(int x) { return (x + 31) / 32 * 32; }
inline bool tq_ok(int tq, int dim_pad) { return tq >= 1 && tq <= SRX_MAXSIM_MAX_QT && ceil32(tq) * dim_pad <= 32768; }
inline int64_t qpack_bytes(int64_t nq, int tq, int dim_pad) { return (nq * ceil32(tq) * dim_pad * 2 + 255) / 256 * 256; }

__device__ __forceinline__ int ms_live_tokens(const MaxsimArgs &a, int q) {
    return a.q_tok_count != nullptr ? min(max(gload_i32(a.q_tok_count + q), 0), a.tq) : a.tq;
}
// the LOCAL doc of position c of query q's list, or -1: padding, at or past the count, outside the index
__device__ __forceinline__ int ms_local_doc(const MaxsimArgs &a, int q, int c) {
    int lim = a.m;
    if (a.cand_count != nullptr) lim = min(lim, max(gload_i32(a.cand_count + q), 0));
    if (c >= lim) return -1;
    const int64_t local = (int64_t)gload_i32(a.cand_doc + (int64_t)q * a.m + c) - a.doc_base;
    return (local >= 0 && local < a.n_docs) ? (int)local : -1;  // n_docs < 2^31
}

// ================================================================================================ pack
// qpack[((q * nab + ab) * ks + s) * 64 + lane] = the rounded columns 16 s + 8 (lane >> 5) .. + 7 of token 32 ab + (lane & 31)
template <int TYPE>
__global__ __launch_bounds__(THREADS) void srx_maxsim_pack_kernel(MaxsimArgs a) {
    const int64_t per_q = (int64_t)a.nab * a.ks * 64, n = (int64_t)a.nq * per_q;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const int lane = (int)(i & 63);
        const int64_t q = i / per_q;
        const int bs = (int)((i - q * per_q) >> 6), ab = bs / a.ks, s = bs - ab * a.ks;
        const int t = ab * 32 + (lane & 31);
        hf_v4i p = {0, 0, 0, 0};
        if (t < a.tq) {
            const hf_v4f *src = reinterpret_cast<const hf_v4f *>(a.q_tok + (q * a.tq + t) * (int64_t)(a.ks * 16) + 16 * s + 8 * (lane >> 5));
            p = hf_round8<TYPE>(src[0], src[1]);
        }
        a.qpack[i] = p;
    }
}

// ================================================================================================ score
template <int TYPE, int NAB>  // NAB: blocks of 32 query tokens (ceil32(tq) / 32)
__global__ __launch_bounds__(THREADS) void srx_maxsim_score_kernel(MaxsimArgs a) {
    extern __shared__ __attribute__((aligned(16))) char ms_smem[];
    hf_v4i *A = reinterpret_cast<hf_v4i *>(ms_smem);  // [NAB][ks][64]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const int q = (int)(blockIdx.x / (unsigned)a.slices), slice = (int)(blockIdx.x - (unsigned)q * (unsigned)a.slices);
    const int ks = a.ks, pieces = NAB * ks * 64;
    const hf_v4i *qp = a.qpack + (int64_t)q * pieces;
    for (int i = tid; i < pieces; i += THREADS) A[i] = qp[i];
    const int live_t = ms_live_tokens(a, q);
    __syncthreads();
    const float NEG_INF = -__builtin_inff();
    const int c0 = slice * MS_SLICE, nc = min(MS_SLICE, a.m - c0);  // c0 < m <= 2^31 - 1: nothing past m is computed
    for (int j = wave; j < nc; j += WAVES) {                        // uniform per wave
        const int c = c0 + j;
        const int local = uni(ms_local_doc(a, q, c));
        float score = 0.0f;
        int t0 = 0, t1 = 0;
        if (local >= 0) {
            t0 = uni(max(gload_i32(a.tok_ptr + local), 0));
            t1 = uni((int)min((int64_t)gload_i32(a.tok_ptr + local + 1), a.n_tok));
        }
        if (t1 > t0 && live_t > 0) {
            const int nblk = (t1 - t0 + 31) >> 5, gpb = ks / MS_G, total = nblk * gpb;
            float mx[NAB][16];
            hf_v16f acc[NAB];
#pragma unroll
            for (int ab = 0; ab < NAB; ++ab)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    mx[ab][e] = NEG_INF;
                    acc[ab][e] = 0.0f;
                }
            hf_v4i pre[MS_G], cur[MS_G];
            // group g: block g / gpb, k-steps (g % gpb) * MS_G .. + MS_G - 1; the lane's token row of the block, zeros past the doc
            auto load_group = [&](int g) __attribute__((always_inline)) {
                const int b = g / gpb, s0 = (g - b * gpb) * MS_G;
                const int off = 32 * b + r;  // < t1 - t0 + 31
                const bool in = off < t1 - t0;
                const hf_v4i *p = a.tok + hf_piece(in ? t0 + off : 0, ks, s0, h);
#pragma unroll
                for (int u = 0; u < MS_G; ++u) {
                    pre[u] = (hf_v4i){0, 0, 0, 0};
                    if (in) pre[u] = p[u * 64];
                }
            };
            load_group(0);
            for (int g = 0; g < total; ++g) {
                const int b = g / gpb, s0 = (g - b * gpb) * MS_G;
#pragma unroll
                for (int u = 0; u < MS_G; ++u) cur[u] = pre[u];
                if (g + 1 < total) load_group(g + 1);  // in flight over this group's MFMAs
#pragma unroll
                for (int u = 0; u < MS_G; ++u)  // ascending k: one chain per output element
#pragma unroll
                    for (int ab = 0; ab < NAB; ++ab) acc[ab] = hf_mfma<TYPE>(A[(ab * ks + s0 + u) * 64 + lane], cur[u], acc[ab]);
                if (s0 + MS_G == ks) {  // the block's chains are complete: column r is doc token t0 + 32 b + r
                    const bool in = 32 * b + r < t1 - t0;
#pragma unroll
                    for (int ab = 0; ab < NAB; ++ab)
#pragma unroll
                        for (int e = 0; e < 16; ++e) {
                            const float v = acc[ab][e];
                            mx[ab][e] = (in && v > mx[ab][e]) ? v : mx[ab][e];
                            acc[ab][e] = 0.0f;
                        }
                }
            }
            // the max over the 32 columns of each half; then row (e & 3) + 8 (e >> 2) + 4 h of block ab is in every lane of half h
#pragma unroll
            for (int ab = 0; ab < NAB; ++ab)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    float v = mx[ab][e];
#pragma unroll
                    for (int o = 16; o > 0; o >>= 1) {
                        const float w = __shfl_xor(v, o);
                        v = w > v ? w : v;
                    }
                    mx[ab][e] = v;
                }
            // the ordered sum: query token i = 32 ab + row, row = (e & 3) + 8 (e >> 2) + 4 h
#pragma unroll
            for (int ab = 0; ab < NAB; ++ab)
#pragma unroll
                for (int row = 0; row < 32; ++row) {
                    const int e = (row & 3) + 4 * (row >> 3), hh = (row >> 2) & 1;
                    const float v = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mx[ab][e]), 32 * hh));
                    if (ab * 32 + row < live_t) score = score + v;
                }
        }
        if (lane == 0) a.score[(int64_t)q * a.m + c] = score;
    }
}

// ================================================================================================ rank
// fp32 total order (finite values, -0 < +0) as unsigned order
__device__ __forceinline__ unsigned ms_order_key(float x) {
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ms_order_value(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key); }

__global__ __launch_bounds__(THREADS) void srx_maxsim_rank_kernel(MaxsimArgs a) {
    __shared__ unsigned long long key[KMAX];
    __shared__ unsigned red[4 * WAVES];
    const int tid = threadIdx.x, q = (int)blockIdx.x, m = a.m, k = a.k;
    unsigned n = 1;
    while (n < (unsigned)m) n <<= 1;  // <= 1024
    unsigned mine = 0;
    for (unsigned i = tid; i < n; i += THREADS) {
        unsigned long long x = 0ull;  // a dead position: below every live key (a live key's low word is >= 1)
        if (i < (unsigned)m && ms_local_doc(a, q, (int)i) >= 0) {
            const int doc = gload_i32(a.cand_doc + (int64_t)q * m + i);  // 0 <= doc <= 2^31 - 2 (doc_base >= 0, local < n_docs)
            x = ((unsigned long long)ms_order_key(a.score[(int64_t)q * m + i]) << 32) | (0x7FFFFFFFu - (unsigned)doc);
            ++mine;
        }
        key[i] = x;
    }
    const unsigned live = block_sum(mine, red);  // ends with a barrier: the keys are in place
    for (unsigned size = 2; size <= n; size <<= 1) {
        for (unsigned stride = size >> 1; stride > 0; stride >>= 1) {
            for (unsigned i = tid; i < (n >> 1); i += THREADS) {
                const unsigned pos = 2 * i - (i & (stride - 1));
                const unsigned long long x = key[pos], y = key[pos + stride];
                const bool desc = (pos & size) == 0;
                if (desc ? (x < y) : (x > y)) {
                    key[pos] = y;
                    key[pos + stride] = x;
                }
            }
            __syncthreads();
        }
    }
    const unsigned cnt = min((unsigned)k, live);
    int32_t *od = a.out_doc + (int64_t)q * k;
    float *os = a.out_score + (int64_t)q * k;
    for (unsigned i = tid; i < (unsigned)k; i += THREADS) {
        if (i < cnt) {
            const unsigned long long x = key[i];
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
template <int TYPE>
void launch_score(const MaxsimArgs &a, hipStream_t stream) {
    const int64_t pieces = (int64_t)a.nq * a.nab * a.ks * 64;
    const int64_t pack_blocks = (pieces + THREADS - 1) / THREADS;
    hipLaunchKernelGGL(srx_maxsim_pack_kernel<TYPE>, dim3((unsigned)(pack_blocks < 65536 ? pack_blocks : 65536)), dim3(THREADS), 0, stream, a);
    const dim3 grid((unsigned)((int64_t)a.nq * a.slices));  // <= nq * m < 2^31
    const size_t lds = (size_t)a.nab * a.ks * 64 * 16;      // <= MS_LDS_MAX
#define SRX_MS(NAB)                                                                                              \
    if (a.nab == NAB) {                                                                                          \
        hipLaunchKernelGGL((srx_maxsim_score_kernel<TYPE, NAB>), grid, dim3(THREADS), lds, stream, a);          \
        return;                                                                                                  \
    }
    SRX_MS(1) SRX_MS(2) SRX_MS(3) SRX_MS(4)
#undef SRX_MS
}

// k < 0: the scorer form
int maxsim_run(const char *who, int32_t device, int32_t type, const void *tok_packed, int64_t n_tok, int32_t dim_pad, const int32_t *tok_ptr,
               int64_t n_docs, int64_t doc_base, const float *q_tok, const int32_t *q_tok_count, int32_t nq, int32_t tq, const int32_t *cand_doc,
               const int32_t *cand_count, int32_t m, int32_t k, int32_t *out_doc, float *out_score, int32_t *out_count, void *workspace,
               int64_t workspace_bytes, void *stream_v) {
    const bool rerank = k >= 0;
    if (type != SRX_HALF_F16 && type != SRX_HALF_BF16) return fail(SRX_ERR_INVALID, "%s: type must be SRX_HALF_F16 or SRX_HALF_BF16", who);
    if (!hf_dim_ok(dim_pad)) return fail(SRX_ERR_INVALID, "%s: dim_pad must be a multiple of 64, <= 1024 (pad the rows with zeros)", who);
    if (!tq_ok(tq, dim_pad)) return fail(SRX_ERR_INVALID, "%s: tq must be in 1 .. 128 with ceil32(tq) * dim_pad <= 32768", who);
    if (m < 1) return fail(SRX_ERR_INVALID, "%s: m must be >= 1", who);
    if (rerank && m > KMAX) return fail(SRX_ERR_INVALID, "%s: m must be in 1 .. 1024", who);
    if (rerank && (k < 1 || k > m)) return fail(SRX_ERR_INVALID, "%s: k must be in 1 .. m", who);
    if (n_docs <= 0 || n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: n_docs out of range", who);
    if (n_tok < 0 || n_tok >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: n_tok out of range", who);
    if (doc_base < 0) return fail(SRX_ERR_INVALID, "%s: doc_base < 0", who);
    if (nq < 0) return fail(SRX_ERR_INVALID, "%s: nq < 0", who);
    if ((int64_t)nq * (int64_t)m > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: nq * m must fit int32", who);
    if (nq == 0) return SRX_OK;
    if (!tok_ptr || !q_tok || !cand_doc || !out_score || (n_tok > 0 && !tok_packed)) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (rerank && (!out_doc || !out_count)) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if (((uintptr_t)tok_packed | (uintptr_t)q_tok) & 15) return fail(SRX_ERR_INVALID, "%s: tok_packed / q_tok must be 16-byte aligned", who);
    const int64_t qbytes = qpack_bytes(nq, tq, dim_pad);
    const int64_t need = qbytes + (rerank ? ((int64_t)nq * m * 4 + 255) / 256 * 256 : 0) + 256;
    if (!workspace || workspace_bytes < need) return fail(SRX_ERR_NOMEM, "%s: workspace too small", who);
    HIP_TRY(hipSetDevice(device));
    char *base = (char *)(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    MaxsimArgs a = {};
    a.tok = (const hf_v4i *)tok_packed;
    a.tok_ptr = tok_ptr;
    a.q_tok = q_tok;
    a.q_tok_count = q_tok_count;
    a.cand_doc = cand_doc;
    a.cand_count = cand_count;
    a.qpack = (hf_v4i *)base;
    a.score = rerank ? (float *)(base + qbytes) : out_score;
    a.out_doc = out_doc;
    a.out_score = out_score;
    a.out_count = out_count;
    a.n_tok = n_tok;
    a.n_docs = n_docs;
    a.doc_base = doc_base;
    a.nq = nq;
    a.tq = tq;
    a.nab = ceil32(tq) / 32;
    a.ks = dim_pad / 16;
    a.m = m;
    a.k = k;
    a.slices = (int)(((int64_t)m + MS_SLICE - 1) / MS_SLICE);
    hipStream_t stream = (hipStream_t)stream_v;
    if (type == SRX_HALF_F16)
        launch_score<SRX_HALF_F16>(a, stream);
    else
        launch_score<SRX_HALF_BF16>(a, stream);
    HIP_TRY(hipGetLastError());
    if (rerank) {
        hipLaunchKernelGGL(srx_maxsim_rank_kernel, dim3((unsigned)nq), dim3(THREADS), 0, stream, a);
        HIP_TRY(hipGetLastError());
    }
    return SRX_OK;
}

}  // namespace

SRX_API int64_t srx_maxsim_workspace_bytes(int32_t nq, int32_t tq, int32_t dim_pad, int32_t m) {
    if (nq < 0 || !hf_dim_ok(dim_pad) || !tq_ok(tq, dim_pad) || m < 0 || m > KMAX || (int64_t)nq * (int64_t)m > 0x7FFFFFFFll)
        return fail(SRX_ERR_INVALID, "srx_maxsim_workspace_bytes: need nq >= 0, tq in 1 .. 128 with ceil32(tq) * dim_pad <= 32768, m in 0 .. 1024%s");
    return qpack_bytes(nq, tq, dim_pad) + (m > 0 ? ((int64_t)nq * m * 4 + 255) / 256 * 256 : 0) + 256;
}

SRX_API int srx_maxsim_score_docs_half(int32_t device, int32_t type, const void *tok_packed, int64_t n_tok, int32_t dim_pad,
                                       const int32_t *tok_ptr, int64_t n_docs, int64_t doc_base, const float *q_tok,
                                       const int32_t *q_tok_count, int32_t nq, int32_t tq, const int32_t *cand_doc, const int32_t *cand_count,
                                       int32_t m, float *out_score, void *workspace, int64_t workspace_bytes, void *stream) {
    return maxsim_run("srx_maxsim_score_docs_half", device, type, tok_packed, n_tok, dim_pad, tok_ptr, n_docs, doc_base, q_tok, q_tok_count, nq, tq,
                      cand_doc, cand_count, m, -1, nullptr, out_score, nullptr, workspace, workspace_bytes, stream);
}

SRX_API int srx_maxsim_rerank_half(int32_t device, int32_t type, const void *tok_packed, int64_t n_tok, int32_t dim_pad,
                                   const int32_t *tok_ptr, int64_t n_docs, int64_t doc_base, const float *q_tok, const int32_t *q_tok_count,
                                   int32_t nq, int32_t tq, const int32_t *cand_doc, const int32_t *cand_count, int32_t m, int32_t k,
                                   int32_t *out_doc, float *out_score, int32_t *out_count, void *workspace, int64_t workspace_bytes,
                                   void *stream) {
    if (k < 0) return fail(SRX_ERR_INVALID, "%s: k must be in 1 .. m", "srx_maxsim_rerank_half");
    return maxsim_run("srx_maxsim_rerank_half", device, type, tok_packed, n_tok, dim_pad, tok_ptr, n_docs, doc_base, q_tok, q_tok_count, nq, tq,
                      cand_doc, cand_count, m, k, out_doc, out_score, out_count, workspace, workspace_bytes, stream);
}
