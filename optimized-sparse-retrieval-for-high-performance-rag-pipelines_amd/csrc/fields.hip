// fields.hip -- field predicates (sparse_rx_fields.h): filter rows built from resident metadata columns.  Row r allows doc d iff
// the base row allows it, every clause of all[r] holds for d, one clause of any[r] (when the list is not empty) and no clause of
// none[r]; a clause is a typed test (range, member of a list, bit mask) on the value d has in one column.
//
// Replaces nothing in the reference project: it has no filters.
//
// A streaming kernel without LDS and without atomics.  One workgroup per (chunk of FD_CHUNK_DOCS = 2048 docs, batch of rows):
// a chunk starts on a 128-doc boundary, so its slice of a row is 64 words = whole 16-byte pieces, and a row's length
// (a multiple of 4 words) ends on one of them -- the padding words of a row are the tail of its last chunk's slice and need
// no path of their own.  Each of the 4 waves owns 512 docs of the chunk = FD_STEPS = 8 steps of 64 docs.  In step s lane l
// looks at doc d_wave + 64 s + l: a clause's column load is one contiguous piece of memory, and __ballot of the lanes'
// verdicts is the clause's 64 doc bits of the step.  The ballot of step s is deposited in lane s >> 1: lane j keeps the four words
// of steps 2 j and 2 j + 1, which are the 16 bytes it stores.  So the masks of a wave's 8 steps are four VGPRs of lanes 0..3,
// and the row's lists fold them with four VALU operations each:
//     acc = (docs below n_docs) & the base row's words;  all: acc &= m;  any: acc &= (m | m' | ..);  none: acc &= ~m.
// Base and validity words are read as the same 16 bytes per lane.  One 16-byte store per lane: 64 contiguous bytes per wave, 256
// per workgroup and row; every word is stored exactly once.
//
// A clause is evaluated for the wave's 8 steps at once: its id, its record and its column descriptor are fetched once, and the 8
// column loads are independent, so they are in flight together.  (Step by step, with each clause of each step a chain of four
// dependent loads, the kernel measured 2.5 times slower at 10 M docs.)  Once the wave's masks of a row
// are all zero the remaining clauses of the row are skipped; the zeros are still stored.
//
// The workgroup loops over the rows of its batch: the chunk's column values come from HBM once, later rows find them in the
// caches.  rows per batch = chunks / FD_CHUNKS_PER_ROW, at least 1 and at most FD_MAX_BATCH_ROWS: with few chunks the rows supply
// the workgroups (batches of one row); with many, batches of 16 rows keep enough batches of ONE chunk in flight together that
// its values are shared in L2 (see the kernel).  Grid y is the batches, capped at 65 535 with a loop beyond.
//
// What is the same in every lane -- clause ids and records, list pointers, IN values, column descriptors, the base row of an
// output row -- is read through the constant address space (cload_*, srx_common.h): scalar loads, no VGPR load per lane.  The
// column descriptors travel as a kernel argument.
//
// A clause id outside [0, n_clauses), a col outside [0, n_cols) and an op that does not fit the column's type give "no doc":
// -1 is the legal spelling of the first, the others are precondition violations that the kernel does not turn into a wild read.
//
// This unit also defines the host checks of field_common.h, which the units over these columns share.
#include "field_common.h"

namespace {

constexpr int FD_CHUNK_DOCS = 2048;                      // docs per workgroup: a multiple of 128
constexpr int FD_CHUNK_WORDS = FD_CHUNK_DOCS / 32;       // 64
constexpr int FD_STEPS = FD_CHUNK_DOCS / (WAVES * 64);   // 8 steps of 64 docs per wave
constexpr int FD_WAVE_WORDS = FD_STEPS * 2;              // 16 words = 4 lanes of 16 bytes
constexpr int FD_MAX_COLS = 32;
constexpr int FD_CHUNKS_PER_ROW = 8;                     // rows per batch = chunks / 8, at least 1 ...
constexpr int FD_MAX_BATCH_ROWS = 16;                    // ... and at most 16
constexpr int FD_MAX_ROWS_Y = 65535;                     // grid.y; more batches than that are looped over

struct FieldsArgs {
    srx_field_col cols[FD_MAX_COLS];
    const srx_field_clause *clauses;
    const int64_t *values;
    const int32_t *lptr[3], *lclause[3];  // all, any, none
    const uint32_t *base_bits;            // null: every doc
    const int32_t *base_q;                // null: base row 0
    uint32_t *out;
    int64_t n_docs, words;
    int n_cols, n_clauses, n_rows, batch_rows, n_batches;
};

// the 64 doc bits of step s go to lane s >> 1: steps 2 j and 2 j + 1 are the four words lane j stores
__device__ __forceinline__ void deposit(uint4 &k, int lane, int s, uint64_t bits) {
    const bool mine = lane == (s >> 1);
    if (s & 1) {
        k.z = mine ? (uint32_t)bits : k.z;
        k.w = mine ? (uint32_t)(bits >> 32) : k.w;
    } else {
        k.x = mine ? (uint32_t)bits : k.x;
        k.y = mine ? (uint32_t)(bits >> 32) : k.y;
    }
}

// The doc bits of clause c for the wave's FD_STEPS steps, as the words the lanes store (lane j: steps 2 j and 2 j + 1; the other
// lanes: zeros).  The record and the column descriptor are fetched once for all steps, and the steps' column loads are
// independent of each other: they are in flight together.  In step s lane l tests doc d_lane + 64 s, clamped to n_docs - 1 (the
// caller masks the tail); w_lane = the lane's first word of a row, `stores` = the lane owns words of the row.
__device__ __forceinline__ uint4 clause_docs(const FieldsArgs &a, int c, int lane, uint32_t d_lane, int64_t w_lane, bool stores) {
    uint4 m = make_uint4(0u, 0u, 0u, 0u);
    if (c < 0 || c >= a.n_clauses) return m;
    const srx_field_clause *rec = a.clauses + c;
    const int col = cload_i32(&rec->col), op = cload_i32(&rec->op);
    if (col < 0 || col >= a.n_cols) return m;
    const int64_t lo = cload_i64(&rec->lo), hi = cload_i64(&rec->hi);
    const void *data = a.cols[col].data;
    const uint32_t *valid = a.cols[col].valid;
    const int type = a.cols[col].type;
    const uint32_t d_last = (uint32_t)(a.n_docs - 1);
    uint32_t d[FD_STEPS];  // doc indices are 32-bit (n_docs < 2^31, and a chunk's tail lies below 2^31 + 2048): one v_min and one shift-add per load
#pragma unroll
    for (int s = 0; s < FD_STEPS; ++s) d[s] = min(d_lane + 64u * s, d_last);
    if (type == SRX_FIELD_I32 || type == SRX_FIELD_I64) {
        if (op != SRX_FOP_RANGE && op != SRX_FOP_IN) return m;
        int64_t v[FD_STEPS];
        if (type == SRX_FIELD_I32) {
#pragma unroll
            for (int s = 0; s < FD_STEPS; ++s) v[s] = (int64_t)srx_field_i32(data, d[s]);
        } else {
#pragma unroll
            for (int s = 0; s < FD_STEPS; ++s) v[s] = srx_field_i64(data, d[s]);
        }
        if (op == SRX_FOP_RANGE) {
#pragma unroll
            for (int s = 0; s < FD_STEPS; ++s) deposit(m, lane, s, __ballot(lo <= v[s] && v[s] <= hi));
        } else {
            bool in[FD_STEPS];
#pragma unroll
            for (int s = 0; s < FD_STEPS; ++s) in[s] = false;
            for (int64_t j = 0; j < hi; ++j) {
                const int64_t x = cload_i64(a.values + lo + j);
#pragma unroll
                for (int s = 0; s < FD_STEPS; ++s) in[s] |= v[s] == x;
            }
#pragma unroll
            for (int s = 0; s < FD_STEPS; ++s) deposit(m, lane, s, __ballot(in[s]));
        }
    } else if (type == SRX_FIELD_F32) {
        if (op != SRX_FOP_RANGE && op != SRX_FOP_IN) return m;
        float v[FD_STEPS];
#pragma unroll
        for (int s = 0; s < FD_STEPS; ++s) v[s] = srx_field_f32(data, d[s]);
        if (op == SRX_FOP_RANGE) {
            const float flo = __int_as_float((int)lo), fhi = __int_as_float((int)hi);
#pragma unroll
            for (int s = 0; s < FD_STEPS; ++s) deposit(m, lane, s, __ballot(flo <= v[s] && v[s] <= fhi));
        } else {
            bool in[FD_STEPS];
#pragma unroll
            for (int s = 0; s < FD_STEPS; ++s) in[s] = false;
            for (int64_t j = 0; j < hi; ++j) {
                const float x = __int_as_float((int)cload_i64(a.values + lo + j));
#pragma unroll
                for (int s = 0; s < FD_STEPS; ++s) in[s] |= v[s] == x;
            }
#pragma unroll
            for (int s = 0; s < FD_STEPS; ++s) deposit(m, lane, s, __ballot(in[s]));
        }
    } else if (type == SRX_FIELD_SET64) {
        if (op != SRX_FOP_MASK_ANY && op != SRX_FOP_MASK_ALL) return m;
        const int64_t want = op == SRX_FOP_MASK_ALL ? lo : 0;  // ALL: (v & lo) == lo;  ANY: (v & lo) != 0
        const bool any = op == SRX_FOP_MASK_ANY;
        int64_t v[FD_STEPS];
#pragma unroll
        for (int s = 0; s < FD_STEPS; ++s) v[s] = srx_field_i64(data, d[s]);
#pragma unroll
        for (int s = 0; s < FD_STEPS; ++s) deposit(m, lane, s, __ballot(((v[s] & lo) == want) != any));
    } else {
        return m;
    }
    if (valid != nullptr && stores) {
        const uint4 ok = srx_field_row_words(valid, w_lane);
        m.x &= ok.x, m.y &= ok.y, m.z &= ok.z, m.w &= ok.w;
    }
    return m;
}

__device__ __forceinline__ bool any_bit(const uint4 &k) { return __ballot((k.x | k.y | k.z | k.w) != 0u) != 0ull; }

__global__ __launch_bounds__(THREADS) void srx_fields_kernel(FieldsArgs a) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // the wave index as a scalar: what hangs on it stays uniform
    // Blocks are dispatched x first.  Taken as they are, the blocks in flight at one time would be ~1 800 CHUNKS of one row batch:
    // at 10 M docs and three columns 72 MB of column values, more than the L2s hold (32 MB), re-read for every row.  So the
    // dispatch order is cut the other way: consecutive blocks are the row BATCHES of one chunk, which share its column values in
    // L2 (a placement that only changes speed: every (chunk, batch) pair is still taken exactly once).
    const uint64_t order = blockIdx.x + (uint64_t)gridDim.x * blockIdx.y;
    const int64_t chunk = (int64_t)(order / gridDim.y);
    const int batch0 = (int)(order % gridDim.y);
    const int64_t w_wave = chunk * FD_CHUNK_WORDS + wave * FD_WAVE_WORDS;  // the wave's first word of a row
    const int64_t d_wave = w_wave * 32;
    const uint32_t d_lane = (uint32_t)d_wave + lane;  // < 2^31 + 2048
    const int64_t w_lane = w_wave + 4 * lane;                                            // lanes 0 .. FD_WAVE_WORDS / 4 - 1 store
    const bool stores = lane < FD_WAVE_WORDS / 4 && w_lane < a.words;                    // words is a multiple of 4
    uint4 docs = make_uint4(0u, 0u, 0u, 0u);                                             // the docs below n_docs in the lane's words
    if (stores) docs = make_uint4(srx_filter_word_docs(a.n_docs, w_lane * 32), srx_filter_word_docs(a.n_docs, w_lane * 32 + 32), srx_filter_word_docs(a.n_docs, w_lane * 32 + 64),
                                  srx_filter_word_docs(a.n_docs, w_lane * 32 + 96));
    const bool wave_live = d_wave < a.n_docs;  // uniform; else the wave lies in the tail of the last chunk: zeros
    for (int b = batch0; b < a.n_batches; b += gridDim.y) {
        const int64_t r_last = ((int64_t)b + 1) * a.batch_rows;
        const int r_end = r_last < a.n_rows ? (int)r_last : a.n_rows;
        for (int r = (int)((int64_t)b * a.batch_rows); r < r_end; ++r) {
            uint4 acc = docs;
            if (wave_live) {
                const int br = srx_filter_base_row(a.base_bits, a.base_q, r);
                if (br >= 0 && stores) {
                    const uint4 bw = srx_field_row_words(a.base_bits + (int64_t)br * a.words, w_lane);
                    acc.x &= bw.x, acc.y &= bw.y, acc.z &= bw.z, acc.w &= bw.w;
                }
                int p0[3], p1[3];
#pragma unroll
                for (int l = 0; l < 3; ++l) {
                    p0[l] = p1[l] = 0;
                    if (a.lptr[l] != nullptr) p0[l] = cload_i32(a.lptr[l] + r), p1[l] = cload_i32(a.lptr[l] + r + 1);
                }
                bool live = any_bit(acc);  // uniform: acc may still hold a bit
                for (int i = p0[0]; i < p1[0] && live; ++i) {
                    const uint4 m = clause_docs(a, cload_i32(a.lclause[0] + i), lane, d_lane, w_lane, stores);
                    acc.x &= m.x, acc.y &= m.y, acc.z &= m.z, acc.w &= m.w;
                    live = any_bit(acc);
                }
                if (p1[1] > p0[1] && live) {
                    uint4 one = make_uint4(0u, 0u, 0u, 0u);
                    for (int i = p0[1]; i < p1[1]; ++i) {
                        const uint4 m = clause_docs(a, cload_i32(a.lclause[1] + i), lane, d_lane, w_lane, stores);
                        one.x |= m.x, one.y |= m.y, one.z |= m.z, one.w |= m.w;
                    }
                    acc.x &= one.x, acc.y &= one.y, acc.z &= one.z, acc.w &= one.w;
                    live = any_bit(acc);
                }
                for (int i = p0[2]; i < p1[2] && live; ++i) {
                    const uint4 m = clause_docs(a, cload_i32(a.lclause[2] + i), lane, d_lane, w_lane, stores);
                    acc.x &= ~m.x, acc.y &= ~m.y, acc.z &= ~m.z, acc.w &= ~m.w;
                    live = any_bit(acc);
                }
            }
            if (stores) *reinterpret_cast<uint4 *>(a.out + (int64_t)r * a.words + w_lane) = acc;
        }
    }
}

int refuse(const char *who, const char *what) {  // SRX_ERR_INVALID with the message "who: what"
    snprintf(g_err, sizeof(g_err), "%s: %s", who, what);
    return SRX_ERR_INVALID;
}

}  // namespace

int srx_check_field_cols(const char *who, const srx_field_col *cols, int n, unsigned admit, const char *unadmitted, bool unadmitted_any) {
    for (int i = 0; i < n; ++i) {
        const int t = cols[i].type;
        const bool known = t >= 0 && t < 32 && (SRX_FIELD_TYPES_ALL >> t & 1u);
        if (!known || !(admit >> t & 1u)) return refuse(who, known || unadmitted_any ? unadmitted : "unknown column type");
        if (!cols[i].data) return refuse(who, "a column with null data");
        if ((uintptr_t)cols[i].data & (t == SRX_FIELD_I64 || t == SRX_FIELD_SET64 ? 7 : 3)) return refuse(who, "column data must be aligned for its type");
        if ((uintptr_t)cols[i].valid & 15) return refuse(who, "a validity row must be 16-byte aligned");
    }
    return SRX_OK;
}

int srx_check_field_docs(const char *who, int64_t n_docs, int64_t doc_base, bool bound_ids) {
    if (n_docs < 1 || n_docs > SRX_FILTER_MAX_DOCS) return refuse(who, "n_docs must be in [1, 2^31 - 2]");
    if (doc_base < 0) return refuse(who, "negative doc_base");
    if (bound_ids && doc_base + n_docs >= 0x7FFFFFFFll) return refuse(who, "doc_base + n_docs must be below 2^31 - 1");
    return SRX_OK;
}

int srx_check_list_shape(const char *who, int32_t m, int32_t m_cap, int32_t k) {
    if (m < 1 || m > m_cap) {
        snprintf(g_err, sizeof(g_err), "%s: m must be in [1, %d]", who, m_cap);
        return SRX_ERR_INVALID;
    }
    return k < 1 || k > m ? refuse(who, "k must be in [1, m]") : SRX_OK;
}

int srx_check_lists(const char *who, int32_t nq, int32_t m, const int32_t *cand_doc, const float *cand_score, bool have_outs, const char *null_outs) {
    if (nq < 0) return refuse(who, "nq < 0");
    if ((int64_t)nq * m > 0x7FFFFFFFll) return refuse(who, "nq * m must not exceed 2^31 - 1");
    if (nq == 0) return SRX_LISTS_EMPTY;
    if (!cand_doc || !cand_score) return refuse(who, "null cand_doc / cand_score");
    return have_outs ? SRX_OK : refuse(who, null_outs);
}

SRX_API int srx_filter_from_fields(int32_t device, int64_t n_docs, const srx_field_col *cols, int32_t n_cols, const srx_field_clause *clauses,
                                   int32_t n_clauses, const int64_t *values, int32_t n_rows, const int32_t *all_ptr, const int32_t *all_clause,
                                   const int32_t *any_ptr, const int32_t *any_clause, const int32_t *none_ptr, const int32_t *none_clause,
                                   const srx_doc_filter *base, uint32_t *out_bits, void *stream_v) {
    const char *who = "srx_filter_from_fields";
    int rc = srx_check_field_docs(who, n_docs, 0, false);
    if (rc != SRX_OK) return rc;
    if (n_cols < 1 || n_cols > FD_MAX_COLS) return fail(SRX_ERR_INVALID, "%s: n_cols must be in [1, 32]", who);
    if (!cols) return fail(SRX_ERR_INVALID, "%s: null cols", who);
    rc = srx_check_field_cols(who, cols, n_cols, SRX_FIELD_TYPES_ALL, nullptr);
    if (rc != SRX_OK) return rc;
    if (n_clauses < 0) return fail(SRX_ERR_INVALID, "%s: n_clauses < 0", who);
    if (n_clauses > 0 && !clauses) return fail(SRX_ERR_INVALID, "%s: null clauses", who);
    rc = srx_check_row_builder(who, "clause", n_rows, all_ptr, all_clause, any_ptr, any_clause, none_ptr, none_clause, out_bits, base);
    if (rc != SRX_OK) return rc;
    if (n_rows == 0) return SRX_OK;
    HIP_TRY(hipSetDevice(device));
    FieldsArgs a;
    memset(&a, 0, sizeof(a));
    for (int i = 0; i < n_cols; ++i) a.cols[i] = cols[i];
    a.clauses = clauses;
    a.values = values;
    a.lptr[0] = all_ptr, a.lclause[0] = all_clause;
    a.lptr[1] = any_ptr, a.lclause[1] = any_clause;
    a.lptr[2] = none_ptr, a.lclause[2] = none_clause;
    a.base_bits = base ? base->bits : nullptr;
    a.base_q = base ? base->q_filter : nullptr;
    a.out = out_bits;
    a.n_docs = n_docs;
    a.words = srx_filter_row_words(n_docs);
    a.n_cols = n_cols;
    a.n_clauses = n_clauses;
    a.n_rows = n_rows;
    const int n_chunks = (int)((n_docs + FD_CHUNK_DOCS - 1) / FD_CHUNK_DOCS);  // <= 2^20
    const int per = n_chunks / FD_CHUNKS_PER_ROW;
    a.batch_rows = per < 1 ? 1 : per < FD_MAX_BATCH_ROWS ? per : FD_MAX_BATCH_ROWS;
    a.n_batches = (n_rows + a.batch_rows - 1) / a.batch_rows;
    const unsigned gy = (unsigned)(a.n_batches < FD_MAX_ROWS_Y ? a.n_batches : FD_MAX_ROWS_Y);
    hipLaunchKernelGGL(srx_fields_kernel, dim3((unsigned)n_chunks, gy), dim3(THREADS), 0, (hipStream_t)stream_v, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
