// collapse.hip -- field collapsing (sparse_rx_collapse.h): the first k positions of a ranked list that have fewer than
// per_group earlier positions of their group, the group being the int64 key a resident metadata column holds for the doc.
//
// Replaces nothing in the reference project: it does not group results.
//
// One workgroup per query, one launch per call, no workspace and no global atomics.  Thread t owns the positions
// t, t + NT, t + 2 NT, ... (R of them: the kernel is instantiated for the list depths 64, 256, 1024 and 2048), so the loads
// of cand_doc and the stores of a chunk of NT positions are contiguous.  Three steps:
//
//   gather   every position loads its doc, tests the two liveness rules and gathers its key: one random 4- or 8-byte load
//            and, where the column has a validity row, one word of it.  What a position is goes to LDS as (key, class):
//            class 0 = in no group (dead, or keyless under NULL_DROP), 1 = has a key, 2 = keyless.  A keyless position takes
//            its own position as key under NULL_OWN (no other position has it: a group of one) and 0 under NULL_ONE (all of
//            them: one group), so that ONE rule -- same class and same key -- is the group of all three policies.
//   walk     position i counts the positions j of its group, all of them (the group's size) and those with j < i (its rank in
//            the group).  The loop runs over j; every lane reads the same LDS address, which is a broadcast without bank
//            conflicts, and compares it with the R keys it holds in registers: m LDS reads and m R compares per thread, m^2
//            compares per query.  The loop is cut at the chunk borders, so that "j < i" is a compare only for the thread's one
//            position of j's own chunk.  i survives iff its class is not 0 and its rank is below per_group.
//   compact  per chunk of NT positions a ballot per wave; the waves' survivor counts go through LDS, every thread sums the
//            counts in front of its (chunk, wave) and adds its rank among the wave's survivors: the survivor's place t in
//            list order.  Places below k are stored, the tail of the row from min(k, survivors) on is padded.
//
// A list of at most 64 positions is one wavefront: its barriers are wave barriers.
//
// The checks of the column, of n_docs / doc_base and of the lists, the validity bit and the column load are field_common.h's.
#include "field_common.h"
#include "sparse_rx_collapse.h"

namespace {

constexpr int CL_MAX_M = SRX_COLLAPSE_MAX_M;

struct CollapseArgs {
    const void *data;            // the column: i32[n_docs] or i64[n_docs]
    const uint32_t *valid;       // one filter row, or null
    const int32_t *cand_doc;     // [nq][m]
    const float *cand_score;     // [nq][m]
    const int32_t *cand_count;   // [nq] or null
    int32_t *out_doc;            // [nq][k]
    float *out_score;            // [nq][k]
    int32_t *out_count;          // [nq]
    int32_t *out_pos;            // [nq][k] or null
    int32_t *out_group;          // [nq][k] or null
    int64_t n_docs, doc_base;
    int m, k, per_group, null_policy, wide;  // wide: the column is I64
};

template <int NT>
__device__ __forceinline__ void cl_sync() {
    if constexpr (NT == 64) wsync(); else __syncthreads();
}

template <int NT, int R>
__global__ __launch_bounds__(NT) void srx_collapse_kernel(CollapseArgs a) {
    constexpr int NW = NT / 64;
    __shared__ int64_t s_key[NT * R];
    __shared__ unsigned char s_cls[NT * R];
    __shared__ int s_cnt[R * NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int m = a.m, k = a.k;
    int n = a.cand_count != nullptr ? cload_i32(a.cand_count + q) : m;  // the live prefix of the list
    n = n < 0 ? 0 : n > m ? m : n;
    const int32_t *row_doc = a.cand_doc + q * m;

    // ---- gather
    int doc[R];
    int64_t key[R];
    int cls[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = tid + r * NT;
        doc[r] = -1, key[r] = 0, cls[r] = 0;
        if (i < n) {  // i < n <= m: inside the row
            doc[r] = gload_i32(row_doc + i);
            const int64_t local = (int64_t)doc[r] - a.doc_base;
            if (local >= 0 && local < a.n_docs) {
                bool has = true;
                if (a.valid != nullptr) has = srx_field_valid_bit(a.valid, local);
                if (has) {
                    cls[r] = 1;
                    key[r] = srx_field_load(a.data, a.wide, false, local);
                } else if (a.null_policy != SRX_COLLAPSE_NULL_DROP) {
                    cls[r] = 2;
                    key[r] = a.null_policy == SRX_COLLAPSE_NULL_OWN ? (int64_t)i : 0;
                }
            }
        }
        if (i < m) {  // i < NT * R: inside the arrays
            s_key[i] = key[r];
            s_cls[i] = (unsigned char)cls[r];
        }
    }
    cl_sync<NT>();

    // ---- walk: all[r] = positions of i's group, before[r] = those in front of i
    int all[R], before[R];
#pragma unroll
    for (int r = 0; r < R; ++r) all[r] = before[r] = 0;
    // chunk c of the list lies in front of every position of a later chunk and behind every position of an earlier one: only
    // the thread's position of chunk c itself has to compare j with its own place
#pragma unroll
    for (int c = 0; c < R; ++c) {
        const int j1 = n < (c + 1) * NT ? n : (c + 1) * NT;
#pragma unroll 2
        for (int j = c * NT; j < j1; ++j) {
            const int64_t kj = s_key[j];
            const int cj = s_cls[j];
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int same = (kj == key[r]) & (cj == cls[r]);
                all[r] += same;
                if (r > c) before[r] += same;
                if (r == c) before[r] += same & (j < tid + c * NT);
            }
        }
    }

    // ---- compact
    unsigned rank[R];
    bool keep[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        keep[r] = cls[r] != 0 && before[r] < a.per_group;
        const unsigned long long b = __ballot(keep[r]);
        rank[r] = lane_rank(b);
        if (lane == 0) s_cnt[r * NW + wave] = __popcll(b);
    }
    cl_sync<NT>();
    int base[R], total = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        base[r] = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            if (w == wave) base[r] = total;
            total += s_cnt[r * NW + w];
        }
    }
    const int64_t o = q * k;
    const uint32_t *row_bits = (const uint32_t *)(a.cand_score + q * m);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int t = base[r] + (int)rank[r];
        if (keep[r] && t < k) {  // t < k: inside the output row; keep: tid + r NT < n <= m
            const int i = tid + r * NT;
            a.out_doc[o + t] = doc[r];
            ((uint32_t *)a.out_score)[o + t] = (uint32_t)gload_i32((const int32_t *)row_bits + i);
            if (a.out_pos != nullptr) a.out_pos[o + t] = i;
            if (a.out_group != nullptr) a.out_group[o + t] = all[r];
        }
    }
    const int cnt = total < k ? total : k;
    for (int t = cnt + tid; t < k; t += NT) {
        a.out_doc[o + t] = -1;
        a.out_score[o + t] = 0.0f;
        if (a.out_pos != nullptr) a.out_pos[o + t] = -1;
        if (a.out_group != nullptr) a.out_group[o + t] = 0;
    }
    if (tid == 0) a.out_count[q] = cnt;
}

}  // namespace

SRX_API int srx_collapse_topk(int32_t device, const srx_field_col *col, int64_t n_docs, int64_t doc_base, const int32_t *cand_doc,
                              const float *cand_score, const int32_t *cand_count, int32_t nq, int32_t m, int32_t k, int32_t per_group,
                              int32_t null_policy, int32_t *out_doc, float *out_score, int32_t *out_count, int32_t *out_pos,
                              int32_t *out_group_size, void *stream_v) {
    const char *who = "srx_collapse_topk";
    if (!col) return fail(SRX_ERR_INVALID, "%s: null col", who);
    int rc = srx_check_field_cols(who, col, 1, SRX_FIELD_TYPES_INT,
                                  "the column must be SRX_FIELD_I32 or SRX_FIELD_I64 (F32 and SET64 columns are no group keys)", true);
    if (rc == SRX_OK) rc = srx_check_field_docs(who, n_docs, doc_base, false);
    if (rc == SRX_OK) rc = srx_check_list_shape(who, m, CL_MAX_M, k);
    if (rc != SRX_OK) return rc;
    if (per_group < 1) return fail(SRX_ERR_INVALID, "%s: per_group must be >= 1", who);
    if (null_policy != SRX_COLLAPSE_NULL_OWN && null_policy != SRX_COLLAPSE_NULL_ONE && null_policy != SRX_COLLAPSE_NULL_DROP)
        return fail(SRX_ERR_INVALID, "%s: unknown null_policy", who);
    rc = srx_check_lists(who, nq, m, cand_doc, cand_score, out_doc && out_score && out_count, "null out_doc / out_score / out_count");
    if (rc != SRX_OK) return rc < 0 ? rc : SRX_OK;  // SRX_LISTS_EMPTY: nothing to do
    HIP_TRY(hipSetDevice(device));
    CollapseArgs a;
    a.data = col->data, a.valid = col->valid;
    a.cand_doc = cand_doc, a.cand_score = cand_score, a.cand_count = cand_count;
    a.out_doc = out_doc, a.out_score = out_score, a.out_count = out_count, a.out_pos = out_pos, a.out_group = out_group_size;
    a.n_docs = n_docs, a.doc_base = doc_base;
    a.m = m, a.k = k, a.per_group = per_group, a.null_policy = null_policy, a.wide = col->type == SRX_FIELD_I64;
    const dim3 grid((unsigned)nq);
    hipStream_t stream = (hipStream_t)stream_v;
    if (m <= 64) hipLaunchKernelGGL((srx_collapse_kernel<64, 1>), grid, dim3(64), 0, stream, a);
    else if (m <= THREADS) hipLaunchKernelGGL((srx_collapse_kernel<THREADS, 1>), grid, dim3(THREADS), 0, stream, a);
    else if (m <= 4 * THREADS) hipLaunchKernelGGL((srx_collapse_kernel<THREADS, 4>), grid, dim3(THREADS), 0, stream, a);
    else hipLaunchKernelGGL((srx_collapse_kernel<THREADS, 8>), grid, dim3(THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
