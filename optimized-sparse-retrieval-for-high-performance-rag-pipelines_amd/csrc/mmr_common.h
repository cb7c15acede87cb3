// mmr_common.h -- internal declarations of the MMR selection (include/sparse_rx_mmr.h, mmr.hip): the arguments its three
// kernels share and the rule that makes a position of a candidate list live.  A header of its own for the reason
// half_common.h gives: srx_common.h and the kernel files it is hashed with identify the build a profile was taken from, and
// the MMR selection changes nothing in what they compile to.
#pragma once
#include "half_common.h"
#include "sparse_rx_mmr.h"

namespace {

constexpr int MMR_PPL = SRX_MMR_MAX_M / 64;  // positions per lane of the selection wave
constexpr int MMR_RA = 4;                    // rows a wave of the f32 Gram kernel holds as "queries"

struct MmrArgs {
    const void *corpus;  // f32[n_docs][dim], or the packed half corpus
    const int32_t *cand_doc;
    const float *cand_rel;
    const int32_t *cand_count;  // may be null
    float *G;                   // [nq][m][m]
    int32_t *out_doc;
    float *out_rel, *out_mmr;   // out_mmr may be null
    int32_t *out_count;
    int64_t n_docs, doc_base;
    int nq, m, k, dim, sim_mode;  // dim: the padded row length, a multiple of 64
    float w_rel, w_div;
};

// The corpus row of position c of query q's list, or -1: c at or past min(max(cand_count[q], 0), m), an id outside the
// corpus, a NaN relevance.
__device__ __forceinline__ int mmr_row(const MmrArgs &a, int q, int c) {
    int lim = a.m;
    if (a.cand_count != nullptr) lim = min(lim, max(gload_i32(a.cand_count + q), 0));
    if (c >= lim) return -1;
    const int64_t at = (int64_t)q * a.m + c;
    const int64_t local = (int64_t)gload_i32(a.cand_doc + at) - a.doc_base;
    const float rel = a.cand_rel[at];
    return (local >= 0 && local < a.n_docs && rel == rel) ? (int)local : -1;  // n_docs < 2^31
}

inline int64_t mmr_gram_bytes(int64_t nq, int64_t m) { return nq * m * m * 4; }

}  // namespace
