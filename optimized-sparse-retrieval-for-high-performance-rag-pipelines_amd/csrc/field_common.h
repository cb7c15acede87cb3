// field_common.h -- what the translation units over the metadata columns of sparse_rx_fields.h share: fields.hip (which defines the
// host functions), collapse.hip, facets.hip, order.hip and boost.hip.  Host functions with hidden visibility, not part of the C ABI;
// every message starts with the caller's name `who`.  The device helpers serve the kernels that compile to the same code through
// them; one that does not keeps its expression and says so.  Not hashed with the search kernels' sources (see filter_common.h).
#pragma once
#include "filter_common.h"
#include "sparse_rx_fields.h"

constexpr unsigned SRX_FIELD_TYPES_INT = 1u << SRX_FIELD_I32 | 1u << SRX_FIELD_I64;  // sets of column types an entry point admits
constexpr unsigned SRX_FIELD_TYPES_NUMBER = SRX_FIELD_TYPES_INT | 1u << SRX_FIELD_F32;
constexpr unsigned SRX_FIELD_TYPES_ALL = SRX_FIELD_TYPES_NUMBER | 1u << SRX_FIELD_SET64;

// The n columns at `cols` (not null), one after the other: a type of `admit`, data not null and aligned for the type, the validity
// row (or null) 16-byte aligned.  One of the four types outside `admit` is refused with the caller's sentence `unadmitted`, any
// other value as "unknown column type" -- or with that sentence too (`unadmitted_any`: it names the admitted types).
int srx_check_field_cols(const char *who, const srx_field_col *cols, int n, unsigned admit, const char *unadmitted, bool unadmitted_any = false);
// n_docs in [1, 2^31 - 2], doc_base >= 0 and, with `bound_ids`, doc_base + n_docs < 2^31 - 1 (every id of the table is an int32).
// The kernels form doc - doc_base in 64 bits, so the entry points that leave the bound out are safe without it.
int srx_check_field_docs(const char *who, int64_t n_docs, int64_t doc_base, bool bound_ids);
// candidate lists: m in [1, m_cap] and k in [1, m] ...
int srx_check_list_shape(const char *who, int32_t m, int32_t m_cap, int32_t k);
// ... then nq >= 0, nq * m <= 2^31 - 1 and, unless nq == 0, cand_doc / cand_score and the outputs (`have_outs`; `null_outs`: the
// message for one missing).  SRX_OK, a negative code, or SRX_LISTS_EMPTY for nq == 0: nothing to do, the caller returns SRX_OK.
constexpr int SRX_LISTS_EMPTY = 1;
int srx_check_lists(const char *who, int32_t nq, int32_t m, const int32_t *cand_doc, const float *cand_score, bool have_outs, const char *null_outs);

// the validity bit of local doc d (valid is not null; d inside the table)
template <typename I>
__device__ __forceinline__ uint32_t srx_field_valid_bit(const uint32_t *valid, I d) {
    return ((uint32_t)gload_i32((const int32_t *)valid + (d >> 5)) >> (d & 31)) & 1u;
}
// entry d of a column by the type of its entries ...
template <typename I>
__device__ __forceinline__ int32_t srx_field_i32(const void *data, I d) { return ((const SRX_GLOBAL int32_t *)data)[d]; }
template <typename I>
__device__ __forceinline__ int64_t srx_field_i64(const void *data, I d) { return ((const SRX_GLOBAL int64_t *)data)[d]; }
template <typename I>
__device__ __forceinline__ float srx_field_f32(const void *data, I d) { return ((const SRX_GLOBAL float *)data)[d]; }
// ... and as int64 whatever the type: 8-byte entries (I64, SET64: `wide`) as they are, an I32 sign-extended, an F32 (`f32`) as its bits
template <typename I>
__device__ __forceinline__ int64_t srx_field_load(const void *data, bool wide, bool f32, I d) {
    if (wide) return srx_field_i64(data, d);
    const int32_t w = srx_field_i32(data, d);
    return f32 ? (int64_t)(uint32_t)w : (int64_t)w;
}
// a lane's four words of a filter or validity row (w is a multiple of 4 and w + 3 < words: rows are 16-byte aligned)
__device__ __forceinline__ uint4 srx_field_row_words(const uint32_t *row, int64_t w) {
    const srx_i4u v = gload_i4((const int32_t *)(row + w));
    return make_uint4((uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w);
}
