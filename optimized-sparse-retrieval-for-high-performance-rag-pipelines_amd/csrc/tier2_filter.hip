// tier2_filter.hip -- the tier-2 kernel of a filtered search (sparse_rx_filter.h): {f32, f16} x {canonical blocks, compact copy},
// each testing the search-after bound AND the doc filter wherever a candidate is formed.
//
// The kernel is tier2_kernel.hip's, compiled here a second time and not edited: that file is one of the four whose hash names
// the build a profile was taken from, and its plain and search-after instances are what every unfiltered search runs -- named
// in one unit with them, filtered instances changed the register allocation of the plain ones (inlining and allocation depend
// on every instance a unit names).  What this unit adds around the included text:
//
//   * the predicate.  tier2_kernel.hip funnels every candidate (score bits, local doc) through after_bound<AFTER>(const
//     ScoreShared &, ...).  Declared BEFORE the include, the overload below takes ScoreShared & -- every call site holds a
//     non-const S, so overload resolution picks it there -- and is: the file's own test, then the doc's filter bit.  Were a call
//     site ever to pass a const S it would silently lose the filter.  tests/test_filter_gpu.py runs sampled corpora and masks
//     against the oracle; tests/test_tier2_filter_routes_cpu.py / _gpu.py run the directed route cases (every path, every
//     selection edge, all four instances) under masks built so that, per step of the restated route, losing the filter inside
//     that step's doc range alone changes the expected rows -- and more work items than workgroups, for the row below.
//   * the work item's filter row, in a workgroup-shared word pair of this unit (FilterItem); srx_filtered_score_kernel resolves
//     it (q_filter, -1, NULL) once per item and calls the file's score_block<VT, true, CP>, whose open_item publishes it with its
//     barriers and sets the bound to "none" (0xFFFFFFFF) when the search carries none.
//   * the launcher of the included file becomes a static function nobody calls, and the launch macro expands to nothing while
//     the file is read, so the eight unfiltered kernels it names are not instantiated a second time.
//
// The bit is one cached global load behind the two LDS reads of the bound test, issued only for candidates that passed
// score > 0, the threshold and the bound (the bitmap is read-only during a search and small: a 10 M-doc row is 1.25 MB, in L2).
//
// Replaces nothing in the reference project: it has no filters.

#include "filter_common.h"

namespace {
struct ScoreShared;
struct FilterItem {
    const unsigned *row;  // the query's filter row (bit d & 31 of word d >> 5: local doc d is allowed); null: not filtered
    int n_docs;           // docs the row has bits for: a dense tile's last accumulators may lie past them
};
__shared__ FilterItem g_filter_item;

template <bool AFTER>
__device__ __forceinline__ bool after_bound(ScoreShared &S, unsigned b, int doc);
}  // namespace

#define srx_launch_score_kernel static __attribute__((unused)) srx_unfiltered_launcher_of_this_unit
#pragma push_macro("hipLaunchKernelGGL")
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(...) ((void)0)
#include "tier2_kernel.hip"
#pragma pop_macro("hipLaunchKernelGGL")
#undef srx_launch_score_kernel

namespace {
template <bool AFTER>
__device__ __forceinline__ bool after_bound(ScoreShared &S, unsigned b, int doc) {
    if (!after_bound<AFTER>(static_cast<const ScoreShared &>(S), b, doc)) return false;  // tier2_kernel.hip's: the bound
    if constexpr (!AFTER) return true;
    const unsigned *row = g_filter_item.row;
    if (row == nullptr) return true;
    return doc < g_filter_item.n_docs && ((row[doc >> 5] >> (doc & 31)) & 1u) != 0u;
}

template <typename VT, bool CP>
__global__ __launch_bounds__(THREADS, 2) void srx_filtered_score_kernel(const srx_score_launch a, const srx_filter_rows f) {
    __shared__ ScoreShared S;
    static_assert(2 * (sizeof(ScoreShared) + sizeof(FilterItem)) <= 160 * 1024, "the launch bounds: two workgroups share a CU's 160 KiB of LDS");
    const int *__restrict__ work = a.w.work;
    const int n_work = work[0];
    if (a.hint != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *a.hint = n_work;
    for (int w = blockIdx.x; w < n_work; w += gridDim.x) {
        __syncthreads();  // the previous item's LDS state is dead, its filter row included
        const int bid = work[1 + w];
        if (threadIdx.x == 0) {
            int q, split, nsq;
            decode_item(bid, a.w.n_whole, a.w.n_splits, q, split, nsq);
            const int r = (q < a.w.nq && f.q_filter != nullptr) ? f.q_filter[q] : 0;
            g_filter_item.row = r < 0 ? nullptr : f.bits + (int64_t)r * f.words;
            g_filter_item.n_docs = (int)a.w.ix.n_docs;
        }
        score_block<VT, true, CP>(S, bid, a);  // open_item's barriers publish the row before the first candidate is formed
    }
}

template <typename VT>
void launch_filtered(const srx_score_launch &a, const srx_filter_rows &f, unsigned grid, hipStream_t stream) {
    if (a.w.ix.post == nullptr)  // no canonical blocks: the compact copy
        hipLaunchKernelGGL((srx_filtered_score_kernel<VT, true>), dim3(grid), dim3(THREADS), 0, stream, a, f);
    else
        hipLaunchKernelGGL((srx_filtered_score_kernel<VT, false>), dim3(grid), dim3(THREADS), 0, stream, a, f);
}
}  // namespace

int srx_launch_filtered_score_kernel(const srx_score_launch &a, const srx_filter_rows &f, int val_type, unsigned grid, hipStream_t stream) {
    val_type == SRX_VAL_F32 ? launch_filtered<float>(a, f, grid, stream) : launch_filtered<__half>(a, f, grid, stream);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}
