// filter_common.h -- what the translation units of a filtered search (sparse_rx_filter.h) share: sparse_rx.hip and dense.hip
// (the drivers), filter.hip (rows, checks, the dense rank kernel), tier2_filter.hip (the filtered tier-2 instances) and the row
// builders terms.hip and fields.hip.  Host functions with hidden visibility, not part of the C ABI.  Kept out of srx_common.h: that header and the three kernel files it
// is hashed with (wave_kernel.hip, tier2_kernel.hip, merge.hip) identify the build a profile was taken from, and a filtered
// search changes nothing in what they compile to.
#pragma once
#include "srx_common.h"
#include "sparse_rx_filter.h"

// words of one filter row: ceil(n_docs / 32) rounded up to a multiple of 4 (srx_filter_words)
inline int64_t srx_filter_row_words(int64_t n_docs) { return ((n_docs + 31) / 32 + 3) / 4 * 4; }

constexpr int64_t SRX_FILTER_MAX_DOCS = 0x7FFFFFFFll - 1;  // n_docs of a filter row, of every index and dense corpus: [1, 2^31 - 2]

// the bits of docs below n_docs in the word that starts at doc d.  fields.hip calls it; the fill and count kernels (filter.hip)
// and the terms kernel keep the expression written out: called from there it is the same value and other gfx950 code.
__host__ __device__ __forceinline__ uint32_t srx_filter_word_docs(int64_t n_docs, int64_t d) {
    const int64_t left = n_docs - d;
    return left >= 32 ? 0xFFFFFFFFu : left > 0 ? (1u << (int)left) - 1u : 0u;
}

// the base row of output row r of a row builder (terms.hip, fields.hip): base_q[r], or row 0 without base_q; < 0 = none (no
// base, or base_q[r] = -1).  The row's number, not its address: a helper that returns base_bits + row * words (null: none) makes
// the callers test a pointer where they tested the number, and both kernels compile to other code.
__device__ __forceinline__ int srx_filter_base_row(const uint32_t *base_bits, const int32_t *base_q, int r) {
    int br = base_bits != nullptr ? 0 : -1;
    if (base_bits != nullptr && base_q != nullptr) br = cload_i32(base_q + r);
    return br;
}

// filter.hip: what every filtered entry point checks of its filter before anything touches a device
int srx_check_filter(const char *who, const srx_doc_filter *f);

// filter.hip: what the srx_filter_from_* entry points check of what they share -- n_rows, the three (ptr, ids) list pairs
// (`ids` is the word their message has for the second array: "term", "clause"), out_bits and base (null: none)
int srx_check_row_builder(const char *who, const char *ids, int32_t n_rows, const int32_t *all_ptr, const int32_t *all_ids,
                          const int32_t *any_ptr, const int32_t *any_ids, const int32_t *none_ptr, const int32_t *none_ids,
                          const uint32_t *out_bits, const srx_doc_filter *base);

// tier2_filter.hip: the tier-2 kernel of a filtered search.  `a` is the descriptor of the search as srx_launch_score_kernel
// takes it (after_doc / after_score given or both null); the filter's rows are over a.w.ix.n_docs local docs.
struct srx_filter_rows {
    const uint32_t *bits;     // rows of `words` words each
    const int32_t *q_filter;  // the row of every query (null: row 0; -1: not filtered)
    int64_t words;
};
int srx_launch_filtered_score_kernel(const srx_score_launch &a, const srx_filter_rows &f, int val_type, unsigned grid, hipStream_t stream);

// filter.hip: the filtered form of the dense side's row ranking (dense.hip, srx_dense_topk_kernel on the score matrix): n_splits
// lists of the k best ALLOWED columns per query into `cand`, unordered, for srx_merge_impl.  Query q of the launch reads
// q_filter at q0 + q.  A kernel of its own in a file of its own: a second caller of the top-k helpers inside dense.hip changes
// what the compiler inlines into the unfiltered kernel.
int srx_launch_filtered_topk(const float *scores, int64_t ld, int64_t n_docs, int nq, int k, int n_splits, int64_t doc_base,
                             const srx_doc_filter &filter, int q0, const srx_rows &cand, hipStream_t stream);
