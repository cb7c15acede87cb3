// merge.hip -- exact top-k merge of candidate lists: the per-split / per-tier lists of one search, the per-shard lists of a
// sharded one, the dense side's per-split lists.  srx_merge_kernel (one workgroup per (query, group of lists), up to 4096
// candidates, tree levels above that) and srx_merge_wave_kernel (one wavefront per query, <= 1024 candidates, k <= 128),
// both ranking by (score desc, doc asc); the srx_merge_topk* entry points of the C ABI.
//
// Replaces fast_topk_selection (rag_system/core/retrieval.py:79-92) over concatenated lists.

#include "srx_common.h"

namespace {

// ------------------------------------------------------------------------------------------------
// Merge kernel: one workgroup per (query, group of lists).  Selects the top-k of up to
// MERGE_NPT*256 candidates; if `final`, ranks them (bitonic sort on (score desc, doc asc)), adds
// doc_base and pads the row.
// ------------------------------------------------------------------------------------------------

// Wave-level final merge for the common small case (n_lists * k <= 1024 candidates per query, k <= 128: the splits /
// tiers of one shard, or 8 shards' top-100): one wavefront per query, no barrier.  The candidates are compacted into
// an LDS list, the exact list selection of tier 1 shrinks it to k and the wave ranks and writes the row.
constexpr int MW_CAP = 1024;
struct MergeWaveShared {
    static constexpr bool HIST_ALIASES_ZEROED_LDS = false;
    unsigned lbits[MW_CAP];
    int ldoc[MW_CAP];
    unsigned hist[256];
    unsigned long long sortkey[128];
};

__global__ __launch_bounds__(THREADS) void srx_merge_wave_kernel(const int32_t *__restrict__ in_doc,
                                                                 const float *__restrict__ in_score,
                                                                 const int32_t *__restrict__ in_count, int nq, int n_lists,
                                                                 int k, int gathered, int64_t row_stride,
                                                                 int64_t cnt_stride, int64_t doc_base,
                                                                 int32_t *__restrict__ out_doc,
                                                                 float *__restrict__ out_score,
                                                                 int32_t *__restrict__ out_count, int64_t out_row_stride,
                                                                 int64_t out_cnt_stride, const int *__restrict__ gate, int q0,
                                                                 int skip_final) {
    __shared__ MergeWaveShared MW[WAVES];
    const int lane = threadIdx.x & 63;
    const int q = q0 + blockIdx.x * WAVES + (threadIdx.x >> 6);  // q0: first query this launch covers (the split ones of a search)
    if (q >= nq) return;
    if (gate != nullptr && *gate == 0) return;  // optional device-side switch (dense fallback pass)
    // skip_final (plain layout only): a negative count in the query's first list marks a row its producer already wrote
    if (skip_final && in_count[(int64_t)q * n_lists * cnt_stride] < 0) return;
    MergeWaveShared &S = MW[threadIdx.x >> 6];
    // list lengths first (one round trip), then every candidate slot of the query in one batch of loads (a second
    // round trip), then a ballot compaction of the positive scores into the LDS list
    for (int l = lane; l < n_lists; l += 64) {
        // layout 0: [nq][n_lists][k] (+ counts [nq][n_lists]); gathered: [n_lists][nq][k] (+ [n_lists][nq])
        const int64_t li = gathered ? ((int64_t)l * nq + q) : ((int64_t)q * n_lists + l);
        S.hist[l] = (unsigned)max(0, min(in_count[li * cnt_stride], k));  // n_lists <= 256 (host check); hist is free until the selection
    }
    wsync();
    constexpr int MW_NPL = MW_CAP / 64;  // candidate slots per lane
    float sc[MW_NPL];
    int dd[MW_NPL];
    const int span = n_lists * k;
#pragma unroll
    for (int j = 0; j < MW_NPL; ++j) {
        const int c = j * 64 + lane;
        sc[j] = 0.0f;
        dd[j] = 0;
        if (c < span) {
            const int l = c / k, r = c - l * k;
            if (r < (int)S.hist[l]) {
                const int64_t li = gathered ? ((int64_t)l * nq + q) : ((int64_t)q * n_lists + l);
                const int64_t a = li * row_stride + r;  // row_stride = k for plain lists, 2k+1 for packed rows
                sc[j] = in_score[a];
                dd[j] = in_doc[a];
            }
        }
    }
    unsigned count = 0;  // wave-uniform
#pragma unroll
    for (int j = 0; j < MW_NPL; ++j) {
        const bool ok = sc[j] > 0.0f;
        const unsigned long long m = __ballot(ok);
        if (ok) {
            const unsigned p = count + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
            S.lbits[p] = __float_as_uint(sc[j]);
            S.ldoc[p] = dd[j];
        }
        count += (unsigned)__popcll(m);
    }
    wsync();
    if (count > (unsigned)k) {
        wave_list_select(S, count, k);
        count = (unsigned)k;
    }
    wave_rank_emit(S, S.sortkey, count, k, doc_base, out_doc + (int64_t)q * out_row_stride, out_score + (int64_t)q * out_row_stride);
    if (lane == 0) out_count[(int64_t)q * out_cnt_stride] = (int)count;
}

__global__ __launch_bounds__(THREADS) void srx_merge_kernel(const int32_t *__restrict__ in_doc,
                                                            const float *__restrict__ in_score,
                                                            const int32_t *__restrict__ in_count, int nq, int n_lists,
                                                            int k, int lists_per_group, int n_groups, int final_pass,
                                                            int gathered, int64_t row_stride, int64_t cnt_stride,
                                                            int64_t doc_base, int32_t *__restrict__ out_doc,
                                                            float *__restrict__ out_score,
                                                            int32_t *__restrict__ out_count, int64_t out_row_stride,
                                                            int64_t out_cnt_stride, const int *__restrict__ gate, int q0, int skip_final) {
    __shared__ MergeShared M;
    const int tid = threadIdx.x;
    const int q = q0 + blockIdx.x / n_groups;
    const int g = blockIdx.x - (q - q0) * n_groups;
    if (q >= nq) return;
    if (gate != nullptr && *gate == 0) return;  // optional device-side switch (dense fallback pass)
    // skip_final (plain layout only): a negative count in the query's first list marks a row its producer already wrote
    if (skip_final && in_count[(int64_t)q * n_lists * cnt_stride] < 0) return;
    const int l0 = g * lists_per_group;
    const int l1 = min(l0 + lists_per_group, n_lists);
    if (tid == 0) {
        M.tk.count = 0;
        M.tk.tau = 0;
    }
    __syncthreads();
    // candidates: flat index c -> (list, rank); lists are dense-packed logically as (l - l0)*k + r
    unsigned ubits[MERGE_NPT];
    int udoc[MERGE_NPT];
    const int span = (l1 - l0) * k;
#pragma unroll
    for (int n = 0; n < MERGE_NPT; ++n) {
        const int c = n * THREADS + tid;
        ubits[n] = 0;
        udoc[n] = 0;
        if (c < span) {
            const int l = l0 + c / k, r = c - (c / k) * k;
            // layout 0: [nq][n_lists][k] (+ counts [nq][n_lists]); gathered: [n_lists][nq][k] (+ [n_lists][nq])
            const int64_t li = gathered ? ((int64_t)l * nq + q) : ((int64_t)q * n_lists + l);
            const int cnt = in_count[li * cnt_stride];
            if (r < cnt) {
                const int64_t a = li * row_stride + r;  // row_stride = k for plain lists, 2k+1 for packed rows
                const float s = in_score[a];
                if (s > 0.0f) {
                    ubits[n] = __float_as_uint(s);
                    udoc[n] = in_doc[a];
                }
            }
        }
    }
    topk_fold<MERGE_NPT, false>(ubits, udoc, k, M.tk, M.hist);
    const unsigned cnt = M.tk.count;
    if (!final_pass) {
        const int64_t o = ((int64_t)q * n_groups + g) * k;
        for (unsigned i = tid; i < cnt; i += THREADS) {
            out_doc[o + i] = M.tk.doc[i];
            out_score[o + i] = __uint_as_float(M.tk.bits[i]);
        }
        if (tid == 0) out_count[(int64_t)q * n_groups + g] = (int)cnt;
        return;
    }
    // rank: bitonic sort, descending on key64 = score bits : (0x7FFFFFFF - doc); final rows may live in a strided (packed) buffer
    block_rank_emit(M.tk, M.sortkey, k, doc_base, out_doc + (int64_t)q * out_row_stride, out_score + (int64_t)q * out_row_stride,
                    out_count + (int64_t)q * out_cnt_stride);
}

}  // namespace

// The last merge level: `lists` lists per query -> the ranked final rows of queries [q0, nq).  One wavefront per query
// when the candidates fit it, else one workgroup (lists * k <= 4096: the callers' tree levels / plan see to that).
int srx_launch_final_merge(const srx_const_rows &in, int nq, int lists, int k, int lay, int64_t doc_base, const srx_rows &out,
                           const int *gate, int q0, int skip_final, bool force_block, hipStream_t stream) {
    const int n = nq - q0;
    if (k <= W_KMAX && (int64_t)lists * k <= MW_CAP && lists <= 256 && !force_block)
        hipLaunchKernelGGL(srx_merge_wave_kernel, dim3((unsigned)((n + WAVES - 1) / WAVES)), dim3(THREADS), 0, stream, in.doc,
                           in.score, in.count, nq, lists, k, lay, in.row_stride, in.cnt_stride, doc_base, out.doc, out.score,
                           out.count, out.row_stride, out.cnt_stride, gate, q0, skip_final);
    else
        hipLaunchKernelGGL(srx_merge_kernel, dim3((unsigned)n), dim3(THREADS), 0, stream, in.doc, in.score, in.count, nq,
                           lists, k, lists, 1, 1, lay, in.row_stride, in.cnt_stride, doc_base, out.doc, out.score, out.count,
                           out.row_stride, out.cnt_stride, gate, q0, skip_final);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

SRX_API int64_t srx_merge_workspace_bytes(int32_t nq, int32_t n_lists, int32_t k) {
    if (nq < 0 || n_lists <= 0 || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "srx_merge_workspace_bytes: bad argument%s");
    const int fan = (MERGE_NPT * THREADS) / k;
    if (n_lists <= fan) return 0;
    // two ping-pong buffers sized for the first reduction level
    const int64_t g = (n_lists + fan - 1) / fan;
    return 2 * ((int64_t)nq * g * k * 8 + (int64_t)nq * g * 4 + 256);
}

int srx_merge_impl(int32_t device, const srx_const_rows &in, int32_t nq, int32_t n_lists, int32_t k, int lay, const srx_rows &out,
                   void *workspace, int64_t workspace_bytes, void *stream_v, const int *gate, int skip_marked) {
    if (nq < 0 || n_lists <= 0 || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "srx_merge_topk: bad argument%s");
    if (nq == 0) return SRX_OK;
    if (!in.doc || !in.score || !in.count || !out.doc || !out.score || !out.count)
        return fail(SRX_ERR_INVALID, "srx_merge_topk: null pointer%s");
    const int64_t need = srx_merge_workspace_bytes(nq, n_lists, k);
    if (skip_marked && (lay != 0 || need > 0)) return fail(SRX_ERR_INVALID, "srx_merge_topk: marked rows need the plain layout and a single pass%s");
    if (need > 0 && (!workspace || workspace_bytes < need)) return fail(SRX_ERR_NOMEM, "srx_merge_topk: workspace too small%s");
    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    const int fan = (MERGE_NPT * THREADS) / k;
    srx_const_rows cur = in;
    int lists = n_lists, level = 0;
    const int64_t half = need / 2;
    while (lists > fan) {  // tree levels: groups of `fan` lists -> one unordered list each (plain layout)
        const int groups = (lists + fan - 1) / fan;
        int32_t *od = (int32_t *)((char *)workspace + (level & 1) * half);
        float *os = (float *)(od + (int64_t)nq * groups * k);
        const srx_rows lvl = srx_plain_rows(od, os, (int32_t *)(os + (int64_t)nq * groups * k), k);
        hipLaunchKernelGGL(srx_merge_kernel, dim3((unsigned)((int64_t)nq * groups)), dim3(THREADS), 0, stream, cur.doc, cur.score,
                           cur.count, nq, lists, k, fan, groups, 0, lay, cur.row_stride, cur.cnt_stride, (int64_t)0, lvl.doc,
                           lvl.score, lvl.count, lvl.row_stride, lvl.cnt_stride, gate, 0, 0);
        HIP_TRY(hipGetLastError());
        lay = 0;
        cur = lvl;
        lists = groups;
        ++level;
    }
    return srx_launch_final_merge(cur, nq, lists, k, lay, (int64_t)0, out, gate, 0, skip_marked, false, stream);
}

SRX_API int srx_merge_topk(int32_t device, const int32_t *in_doc, const float *in_score, const int32_t *in_count,
                           int32_t nq, int32_t n_lists, int32_t k, int32_t gathered, int32_t *out_doc, float *out_score,
                           int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream_v) {
    return srx_merge_impl(device, srx_plain_rows(in_doc, in_score, in_count, k), nq, n_lists, k, gathered ? 1 : 0,
                          srx_plain_rows(out_doc, out_score, out_count, k), workspace, workspace_bytes, stream_v);
}

SRX_API int srx_merge_topk_packed(int32_t device, const int32_t *packed, int32_t nq, int32_t n_lists, int32_t k,
                                  int32_t *out_doc, float *out_score, int32_t *out_count, void *workspace,
                                  int64_t workspace_bytes, void *stream_v) {
    if (!packed || k <= 0) return fail(SRX_ERR_INVALID, "srx_merge_topk_packed: bad argument%s");
    return srx_merge_impl(device, srx_packed_rows<const float>(packed, k), nq, n_lists, k, 1, srx_plain_rows(out_doc, out_score, out_count, k),
                          workspace, workspace_bytes, stream_v);
}

SRX_API int srx_merge_topk_packed_out(int32_t device, const int32_t *packed, int32_t nq, int32_t n_lists, int32_t k,
                                      int32_t *out_packed, void *workspace, int64_t workspace_bytes, void *stream_v) {
    if (!packed || !out_packed || k <= 0) return fail(SRX_ERR_INVALID, "srx_merge_topk_packed_out: bad argument%s");
    return srx_merge_impl(device, srx_packed_rows<const float>(packed, k), nq, n_lists, k, 1, srx_packed_rows<float>(out_packed, k), workspace,
                          workspace_bytes, stream_v);
}
