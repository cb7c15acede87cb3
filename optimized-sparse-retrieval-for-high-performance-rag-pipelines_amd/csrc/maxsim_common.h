// maxsim_common.h -- what the two late-interaction units share: maxsim.hip (scores and the top-k of GIVEN candidates,
// include/sparse_rx_maxsim.h) and maxsim_search.hip (the exhaustive search, include/late/sparse_rx_maxsim_search.h).  The query-token
// pack, its argument struct with the small shape helpers, and the order-preserving fp32 key: one copy of the text, so the rounded
// query tokens and the ranking rule of the search ARE the reranker's.  Included the way mmr_common.h and ivf_probe.h are.
#pragma once
#include "half_common.h"
#include "sparse_rx_maxsim.h"

namespace {

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

// ================================================================================================ the ranking key
// fp32 total order (finite values, -0 < +0) as unsigned order
__device__ __forceinline__ unsigned ms_order_key(float x) {
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float ms_order_value(unsigned key) { return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key); }

}  // namespace
