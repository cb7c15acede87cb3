// half_common.h -- internal declarations of the half-precision dense index (include/sparse_rx_half.h, dense_half.hip): the
// fragment-order layout, the two roundings and the plan of a search.  Kept out of srx_common.h for the reason filter_common.h
// gives: that header and the three kernel files it is hashed with identify the build a profile was taken from, and the
// half-precision index changes nothing in what they compile to.
#pragma once
#include "filter_common.h"
#include "sparse_rx_half.h"
#include "sparse_rx_quant.h"  // SRX_QUANT_NONFINITE: the flag bit of a non-finite row

namespace {

typedef int hf_v4i __attribute__((ext_vector_type(4)));
typedef float hf_v4f __attribute__((ext_vector_type(4)));
typedef float hf_v16f __attribute__((ext_vector_type(16)));
typedef _Float16 hf_v8h __attribute__((ext_vector_type(8)));
typedef __bf16 hf_v8b __attribute__((ext_vector_type(8)));

// ---- layout: 16-byte pieces, one per (tile of 32 rows, k-step of 16 columns, lane) ----
// the piece that holds columns 16 s + 8 h .. + 7 of row `row`, at ks = dim_pad / 16 k-steps per row
__host__ __device__ inline int64_t hf_piece(int64_t row, int ks, int s, int h) { return ((row >> 5) * ks + s) * 64 + (row & 31) + 32 * h; }
inline int64_t hf_tiles(int64_t n_rows) { return (n_rows + 31) / 32; }
inline bool hf_dim_ok(int dim_pad) { return dim_pad >= 64 && dim_pad <= 1024 && dim_pad % 64 == 0; }

// ---- rounding: f32 -> the 16 bits of the type, round to nearest even; bad = the result is not finite ----
template <int TYPE>
__device__ __forceinline__ unsigned hf_round(float x, bool &bad) {
    if constexpr (TYPE == SRX_HALF_F16) {
        const _Float16 v = (_Float16)x;  // v_cvt_f16_f32: nearest even, half subnormals kept
        const unsigned b = (unsigned)__builtin_bit_cast(unsigned short, v);
        bad = bad || (b & 0x7C00u) == 0x7C00u;
        return b;
    } else {
        const unsigned u = __float_as_uint(x);
        if ((u & 0x7F800000u) == 0x7F800000u) {  // inf / NaN (kept a NaN)
            bad = true;
            return (u >> 16) | ((u & 0x007FFFFFu) != 0u ? 0x40u : 0u);
        }
        const unsigned r = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
        bad = bad || (r & 0x7F80u) == 0x7F80u;
        return r;
    }
}
// eight f32 -> one piece
template <int TYPE>
__device__ __forceinline__ hf_v4i hf_round8(const hf_v4f &lo, const hf_v4f &hi) {
    bool bad = false;  // a query's non-finite values stay what they round to
    hf_v4i p;
    p.x = (int)(hf_round<TYPE>(lo.x, bad) | (hf_round<TYPE>(lo.y, bad) << 16));
    p.y = (int)(hf_round<TYPE>(lo.z, bad) | (hf_round<TYPE>(lo.w, bad) << 16));
    p.z = (int)(hf_round<TYPE>(hi.x, bad) | (hf_round<TYPE>(hi.y, bad) << 16));
    p.w = (int)(hf_round<TYPE>(hi.z, bad) | (hf_round<TYPE>(hi.w, bad) << 16));
    return p;
}
// one k-step of the chain: acc += A (32 rows x 16) * B (16 x 32 columns)
template <int TYPE>
__device__ __forceinline__ hf_v16f hf_mfma(const hf_v4i &a, const hf_v4i &b, const hf_v16f &acc) {
    if constexpr (TYPE == SRX_HALF_F16)
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(hf_v8h, a), __builtin_bit_cast(hf_v8h, b), acc, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(hf_v8b, a), __builtin_bit_cast(hf_v8b, b), acc, 0, 0, 0);
}

// ---- the plan of one srx_dense_search_half call: query passes and row splits as dense.hip's dense_plan makes them ----
constexpr int HF_NPT = 16;     // columns per thread and step of the rank kernel
constexpr int HF_QTILE = 128;  // queries and docs per workgroup of the GEMM
struct HalfPlan {
    int QB, qb_max;  // queries per pass: as many as keep the score matrix within 4 GiB, but 32 .. 1024 (so the matrix is 128 bytes
                     // per doc, more than 4 GiB, above 2^25 docs); of the largest pass
    int64_t ld;      // row length of the score matrix
    int ns;          // splits of a score row
};
inline HalfPlan half_plan(int nq, int64_t n_docs, int k) {
    HalfPlan p;
    p.ld = (n_docs + 63) / 64 * 64;
    const int64_t q = (4ll << 30) / (p.ld * 4) / 32 * 32;
    p.QB = (int)(q < 32 ? 32 : q > 1024 ? 1024 : q);
    p.qb_max = nq < p.QB ? nq : p.QB;
    int64_t s = 2048 / (p.qb_max > 0 ? p.qb_max : 1);  // >= 2048 workgroups when the batch is small
    const int64_t by_docs = n_docs / (THREADS * HF_NPT * 4), cap = (MERGE_NPT * THREADS) / (k > 0 ? k : 1);  // one merge level
    if (s > by_docs) s = by_docs;
    if (s > cap) s = cap;
    p.ns = (int)(s < 1 ? 1 : s);
    return p;
}
struct HalfWs {
    hf_v4i *qpack;  // the pass's queries in fragment order, whole workgroup tiles of HF_QTILE (zeros past the pass)
    float *scores;  // [qb_max][ld]
    srx_rows cand;  // [qb_max * ns] lists of k
    int64_t bytes;
};
inline HalfWs half_ws(void *base, const HalfPlan &pl, int k) {
    HalfWs w;
    char *p = (char *)base;
    auto take = [&](int64_t bytes) {
        char *r = p;
        p += (bytes + 255) / 256 * 256;
        return r;
    };
    w.qpack = (hf_v4i *)take((int64_t)((pl.qb_max + HF_QTILE - 1) / HF_QTILE) * HF_QTILE * 1024 * 2);  // dim_pad <= 1024
    w.scores = (float *)take((int64_t)pl.qb_max * pl.ld * 4);
    const int64_t lists = (int64_t)pl.qb_max * pl.ns;
    int32_t *cand_doc = (int32_t *)take(lists * k * 4);
    float *cand_score = (float *)take(lists * k * 4);
    w.cand = srx_plain_rows(cand_doc, cand_score, (int32_t *)take(lists * 4), k);
    w.bytes = (int64_t)(p - (char *)base) + 256;
    return w;
}

}  // namespace
