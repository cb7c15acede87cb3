// sparse_rx.hip -- the driver of libsparse_rx.so: the index handle, the search planner and the srx_search* entry points of
// the C ABI.  No kernel lives here: tier 1 is wave_kernel.hip, tier 2 tier2_kernel.hip, the merge merge.hip, the index build
// build.hip, the dense side dense.hip, hybrid fusion fuse.hip, scores of given docs score_docs.hip; shared primitives in
// srx_common.h.
//
// Hot path replaced (paths relative to the reference project):
//   simd_bm25_score      rag_system/core/retrieval.py:41-76      (doc-major full CSR scan per query)
//   simd_tfidf_score     rag_system/pipeline/evaluate_rag_pipeline.py:95-121
//   fast_topk_selection  rag_system/core/retrieval.py:79-92      (+ score>0 filter :292-296)
//
// Design: the index is term-major with a tile skip table; a term's postings are stored as blocks of 4
// (docs and values side by side), one padded run per unit of <= 49152 docs.  A query's doc range is cut into those
// units.  Two tiers score them, a merge kernel ranks:
//   tier 1  srx_wave_kernel   ONE WAVEFRONT per (query, split), no barriers; flags what it cannot serve (long runs, many
//           multi-term docs, > 64 terms, k > 112) for tier 2.
//   tier 2  srx_score_kernel  a persistent grid of 256-thread workgroups drains the worklist of flagged (query, split)
//           blocks.  Handles everything.
//   merge   srx_merge_kernel / srx_merge_wave_kernel  exact top-k over the per-split / per-tier lists + bitonic rank by
//           (score desc, doc asc).  Queries that tier 1 or tier 2 finished on their own are skipped.

#include "srx_common.h"
#include "filter_common.h"

thread_local char srx_g_err[512] = "";

#define SRX_TRY(expr)                  \
    do {                               \
        const int rc_ = (expr);        \
        if (rc_ != SRX_OK) return rc_; \
    } while (0)

namespace {
// The profiler of a handle: the searches it samples are bracketed with PROF_EVENTS events each, kept in a ring of PROF_SLOTS
// slots; read() averages the steps of the slots filled since the last read.
constexpr int PROF_SLOTS = 256;
constexpr int PROF_EVENTS = 4;  // start, after tier 1, after tier 2, after merge
struct SearchProfile {
    hipEvent_t *ev;    // PROF_SLOTS x PROF_EVENTS events, created lazily
    hipEvent_t *cur;   // the slot of the search being issued; null: that search is not sampled
    int n;             // profiled calls recorded since the last read (<= PROF_SLOTS, then it wraps)
    int64_t calls;     // profiled calls ever recorded
    int64_t searches;  // searches issued while profiling was on (every = N samples every N-th of them)

    int begin(int every) {
        cur = nullptr;
        if (every <= 0 || (searches++ % every) != 0) return SRX_OK;
        if (!ev) {
            ev = new (std::nothrow) hipEvent_t[PROF_EVENTS * PROF_SLOTS];
            if (!ev) return fail(SRX_ERR_NOMEM, "srx_search: host allocation failed%s");
            for (int i = 0; i < PROF_EVENTS * PROF_SLOTS; ++i) HIP_TRY(hipEventCreate(&ev[i]));
        }
        cur = ev + PROF_EVENTS * (int)(calls % PROF_SLOTS);
        return SRX_OK;
    }
    int mark(int i, hipStream_t stream) {
        if (cur) HIP_TRY(hipEventRecord(cur[i], stream));
        return SRX_OK;
    }
    void end() {  // the sampled search was issued whole: its slot counts
        if (!cur) return;
        ++calls;
        if (n < PROF_SLOTS) ++n;
    }
    int read(float *h_ms4) {
        if (n == 0 || !ev) return fail(SRX_ERR_INVALID, "srx_profile_read: no profiled srx_search has run%s");
        static constexpr int FROM[4] = {0, 1, 2, 0}, TO[4] = {1, 2, 3, 3};  // tier 1, tier 2, merge, the whole call
        double acc[4] = {0, 0, 0, 0};
        for (int i = 0; i < n; ++i) {
            const hipEvent_t *e = ev + PROF_EVENTS * (int)((calls - 1 - i) % PROF_SLOTS);
            HIP_TRY(hipEventSynchronize(e[3]));
            for (int j = 0; j < 4; ++j) {
                float ms = 0;
                HIP_TRY(hipEventElapsedTime(&ms, e[FROM[j]], e[TO[j]]));
                acc[j] += ms;
            }
        }
        for (int j = 0; j < 4; ++j) h_ms4[j] = (float)(acc[j] / n);
        const int averaged = n;
        n = 0;
        return averaged;
    }
    void destroy() {
        if (!ev) return;
        for (int i = 0; i < PROF_EVENTS * PROF_SLOTS; ++i) (void)hipEventDestroy(ev[i]);
        delete[] ev;
    }
};
}  // namespace

struct srx_index {
    srx_index_desc d;
    srx_search_opts opts;
    SearchProfile prof;
    int *h_hint;  // pinned, device-mapped word: the tier-2 worklist length of a recent search (sizes the next tier-2 grid)
    int *d_hint;  // its device address
};

SRX_API int srx_version(void) { return SRX_VERSION; }
SRX_API const char *srx_last_error(void) { return g_err; }

SRX_API int srx_limits(int32_t *h_out4) {
    if (!h_out4) return fail(SRX_ERR_INVALID, "srx_limits: null output%s");
    h_out4[0] = KMAX;
    h_out4[1] = SRX_MAX_TILE_LOG2;
    h_out4[2] = HASH_CAP;
    h_out4[3] = THREADS;
    return SRX_OK;
}

SRX_API int srx_device_count(void) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return fail(SRX_ERR_NODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return n;
}

SRX_API int srx_index_create(const srx_index_desc *d, srx_index **out) {
    if (!d || !out) return fail(SRX_ERR_INVALID, "srx_index_create: null argument%s");
    if (d->n_docs <= 0 || d->n_docs >= 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "srx_index_create: n_docs out of range%s");
    if (d->doc_base < 0 || d->doc_base + d->n_docs >= 0x7FFFFFFFll)
        return fail(SRX_ERR_INVALID, "srx_index_create: doc_base + n_docs must fit int32%s");
    if (d->vocab <= 0 || d->nnz < 0) return fail(SRX_ERR_INVALID, "srx_index_create: bad vocab / nnz%s");
    if (d->tile_log2 < 6 || d->tile_log2 > SRX_MAX_TILE_LOG2)
        return fail(SRX_ERR_INVALID, "srx_index_create: tile_log2 must be in [6, 14]%s");
    const int64_t nt = (d->n_docs + (1ll << d->tile_log2) - 1) >> d->tile_log2;
    if (d->n_tiles != nt) return fail(SRX_ERR_INVALID, "srx_index_create: n_tiles != ceil(n_docs / 2^tile_log2)%s");
    if (d->val_type != SRX_VAL_F32 && d->val_type != SRX_VAL_F16) return fail(SRX_ERR_INVALID, "srx_index_create: bad val_type%s");
    if (d->unit_tiles < 1 || d->unit_tiles > MAX_TPS) return fail(SRX_ERR_INVALID, "srx_index_create: unit_tiles must be in [1, 64]%s");
    if (d->n_blocks < 0 || d->n_blocks * 4 < d->nnz) return fail(SRX_ERR_INVALID, "srx_index_create: n_blocks does not cover nnz%s");
    if (!d->term_ptr || !d->tile_skip || !d->idf || (!d->post && !d->post16))
        return fail(SRX_ERR_INVALID, "srx_index_create: null index array%s");
    if (!d->post && ((int64_t)d->unit_tiles << d->tile_log2) > W_UNIT_MAX_DOCS)
        return fail(SRX_ERR_INVALID, "srx_index_create: an index without canonical blocks needs units of <= 49152 docs (the compact copy)%s");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (d->device < 0 || d->device >= ndev) return fail(SRX_ERR_NODEVICE, "srx_index_create: device ordinal not visible%s");
    srx_index *ix = new (std::nothrow) srx_index();  // value-initialised: default options, no events, no hint
    if (!ix) return fail(SRX_ERR_NOMEM, "srx_index_create: host allocation failed%s");
    ix->d = *d;
    // 64 bytes of pinned host memory, created once with the handle (srx_search itself allocates nothing).  Not fatal when
    // it cannot be had: the tier-2 grid then always has its full size.
    int *h = nullptr, *dev = nullptr;
    const bool pinned = hipSetDevice(d->device) == hipSuccess && hipHostMalloc((void **)&h, 64, hipHostMallocMapped) == hipSuccess;
    if (pinned && hipHostGetDevicePointer((void **)&dev, h, 0) == hipSuccess) {
        h[0] = -1;  // unknown
        ix->h_hint = h;
        ix->d_hint = dev;
    } else {
        if (pinned) (void)hipHostFree(h);
        (void)hipGetLastError();
    }
    *out = ix;
    return SRX_OK;
}

SRX_API void srx_index_destroy(srx_index *ix) {
    if (!ix) return;
    ix->prof.destroy();
    if (ix->h_hint) (void)hipHostFree(ix->h_hint);
    delete ix;
}

SRX_API int srx_index_set_opts(srx_index *ix, const srx_search_opts *o) {
    if (!ix || !o) return fail(SRX_ERR_INVALID, "srx_index_set_opts: null argument%s");
    if (o->supertile_log2 != 0 && (o->supertile_log2 < ix->d.tile_log2 || o->supertile_log2 > ix->d.tile_log2 + 6))
        return fail(SRX_ERR_INVALID, "srx_index_set_opts: supertile_log2 must be in [tile_log2, tile_log2+6]%s");
    if (o->unit_tiles < 0 || o->unit_tiles > MAX_TPS) return fail(SRX_ERR_INVALID, "srx_index_set_opts: unit_tiles must be in [0, 64]%s");
    if (o->target_blocks < 0) return fail(SRX_ERR_INVALID, "srx_index_set_opts: target_blocks < 0%s");
    if (o->reserved & ~SRX_DBG_ALL)
        return fail(SRX_ERR_INVALID, "srx_index_set_opts: reserved takes only the bits 8, 16, 128, 256, 2048, 4096, 8192%s");
    ix->opts = *o;
    return SRX_OK;
}

namespace {
struct Plan {
    int tpu, n_super, n_splits, n_whole, ovf_words, lists_per_q;  // tpu = tiles per unit; queries < n_whole are not split
};

// Supertile (unit) = the doc range one tier-1 unit covers (<= W_UNIT_MAX_DOCS docs, the wave bitmap): the unit the
// index's runs were padded for at build time (srx_auto_unit_tiles), unless the options override it (then only tier 2
// can serve the queries).
Plan make_plan(const srx_index *ix, int nq, int k) {
    Plan p;
    const srx_index_desc &d = ix->d;
    int tpu;
    if (ix->opts.unit_tiles > 0) {
        tpu = ix->opts.unit_tiles;  // differs from the index's unit: tier 2 serves everything (tier 1 needs the padded runs)
    } else if (ix->opts.supertile_log2 != 0) {
        tpu = 1 << (ix->opts.supertile_log2 - d.tile_log2);
    } else {
        tpu = d.unit_tiles;  // the unit the index was built (padded) for: srx_auto_unit_tiles at build time
    }
    if (tpu < 1) tpu = 1;
    if (tpu > MAX_TPS) tpu = MAX_TPS;
    p.tpu = tpu;
    p.n_super = (int)((d.n_tiles + tpu - 1) / tpu);
    const int target = ix->opts.target_blocks > 0 ? ix->opts.target_blocks : 3072;  // wave-sized workgroups: 256 CUs x 12 resident waves = one full round (C2, 1 k queries: 3 splits 0.088 ms, 4 splits 0.094 ms)
    int ns = target / (nq > 0 ? nq : 1);
    int n_whole = 0;
    if (nq > target) {
        // More queries than resident waves: whole rounds of unsplit queries, and the last partial round cut finer (its
        // queries in up to 4 doc-range splits), so that the kernel does not end on a few long waves (a 10 k-query batch
        // is 3.26 rounds of 3072: measured 3 % slower per query than 9216 or 12288).
        n_whole = nq / target * target;
        const int tail = nq - n_whole;
        ns = tail > 0 ? target / tail : 1;
        if (ns > 4) ns = 4;
        if (ns < 2) ns = 2;
        if (tail == 0) ns = 1;
    }
    if (ns < 1) ns = 1;
    if (ns > p.n_super) ns = p.n_super;
    const int cap = (MERGE_NPT * THREADS) / (2 * (k > 0 ? k : 1));  // merge takes <= 4096 candidates: 2 tiers x splits x k
    if (ns > cap) ns = cap;
    if (ns < 1) ns = 1;
    if (ns == 1) n_whole = 0;
    p.n_splits = ns;
    p.n_whole = n_whole;
    p.ovf_words = (p.n_super + 31) / 32;
    p.lists_per_q = 2 * ns;  // [0, ns): tier 1, [ns, 2 ns): tier 2
    return p;
}
}  // namespace

namespace {
// The one layout of a search's workspace: the candidate lists of every (query, list), the units each work item left to
// tier 2, then the zeroed words (the split queries' arrival counters and work[0]) and the worklist's entries.
struct SearchWs {
    int32_t *cand_doc;    // [lists][k]
    float *cand_score;    // [lists][k]
    int32_t *cand_count;  // [lists]
    unsigned *ovf;        // [items][ovf_words]
    unsigned *done;       // [nq - n_whole]: arrival counters of the split queries; zeroed together with ...
    int *work;            // ... work[0] = the worklist length; its entries work[1 .. items] follow
    int64_t lists, items;
    int64_t bytes;
};
SearchWs search_ws(void *base, const Plan &p, int nq, int k) {
    SearchWs w;
    w.lists = (int64_t)nq * p.lists_per_q;
    w.items = (int64_t)p.n_whole + (int64_t)(nq - p.n_whole) * p.n_splits;
    w.cand_doc = (int32_t *)base;
    w.cand_score = (float *)(w.cand_doc + w.lists * k);
    w.cand_count = (int32_t *)(w.cand_score + w.lists * k);
    w.ovf = (unsigned *)(w.cand_count + w.lists);
    w.done = w.ovf + w.items * p.ovf_words;
    w.work = (int *)(w.done + (nq - p.n_whole));
    w.bytes = (int64_t)((char *)(w.work + 1 + w.items) - (char *)base) + 256;
    return w;
}
}  // namespace

SRX_API int64_t srx_search_workspace_bytes(const srx_index *ix, int32_t nq, int32_t k) {
    if (!ix || nq < 0 || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "srx_search_workspace_bytes: bad argument%s");
    return search_ws(nullptr, make_plan(ix, nq, k), nq, k).bytes;
}

namespace {
// The index as the kernels see it; without the score bounds for a restricted search -- a search-after, a filtered search -- (they
// assume an unrestricted top-k: a threshold derived from a doc the search may not return would cut docs it may) or on request.
IndexView index_view(const srx_index *ix, bool restricted) {
    const srx_index_desc &d = ix->d;
    IndexView v;
    v.term_ptr = d.term_ptr; v.post = d.post; v.post16 = d.post16; v.tile_skip = d.tile_skip; v.idf = d.idf;
    v.term_bound = ((ix->opts.reserved & SRX_DBG_NO_TERM_BOUND) || restricted) ? nullptr : d.term_bound;
    v.n_docs = d.n_docs; v.vocab = d.vocab; v.zero_block = d.n_blocks;
    v.tile_log2 = d.tile_log2; v.n_tiles = d.n_tiles; v.unit_tiles = d.unit_tiles;
    return v;
}

int search_impl(srx_index *ix, const int32_t *q_ptr, const int32_t *q_term, const float *q_weight, int32_t nq,
                int32_t k, const srx_rows &out, void *workspace, int64_t workspace_bytes, void *stream_v,
                const int32_t *after_doc = nullptr, const float *after_score = nullptr, const srx_doc_filter *filter = nullptr) {
    if (!ix) return fail(SRX_ERR_INVALID, "srx_search: null index%s");
    if ((after_doc == nullptr) != (after_score == nullptr)) return fail(SRX_ERR_INVALID, "srx_search_after: after_doc and after_score go together%s");
    if (nq < 0 || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "srx_search: need nq >= 0 and 1 <= k <= 1024%s");
    if (nq == 0) return SRX_OK;
    if (!q_ptr || !out.doc || !out.score || !out.count) return fail(SRX_ERR_INVALID, "srx_search: null query / output pointer%s");
    const Plan p = make_plan(ix, nq, k);
    const SearchWs w = search_ws(workspace, p, nq, k);  // w.items work items: one per unsplit query, n_splits per split query
    if (!workspace || workspace_bytes < w.bytes) return fail(SRX_ERR_NOMEM, "srx_search: workspace too small%s");
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipSetDevice(ix->d.device));
    if (ix->d.post == nullptr && p.tpu != ix->d.unit_tiles)
        return fail(SRX_ERR_INVALID, "srx_search: this index keeps no canonical blocks: a unit other than the one it was built for cannot be served%s");
    if (w.lists > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "srx_search: nq * splits overflows the grid%s");

    // Everything goes to tier 2: by request, for a search-after or a filtered search (the tier-2 kernel applies the bound and
    // the filter), and with another unit than the padded one (tier 1 needs the padded runs).
    const bool restricted = after_score != nullptr || filter != nullptr;
    const bool tier2_only = (ix->opts.reserved & SRX_DBG_TIER2_ONLY) != 0 || restricted || p.tpu != ix->d.unit_tiles;
    srx_score_launch sl;  // one descriptor of the search: tier 1 takes sl.w, tier 2 all of it
    srx_wave_launch &a = sl.w;
    a.ix = index_view(ix, restricted);
    a.q_ptr = q_ptr; a.q_term = q_term; a.q_weight = q_weight;
    a.nq = nq; a.k = k; a.n_splits = p.n_splits; a.n_whole = p.n_whole; a.n_super = p.n_super;
    a.dbg = ix->opts.reserved | (tier2_only ? SRX_DBG_TIER2_ONLY : 0);
    a.ovf = w.ovf; a.ovf_words = p.ovf_words; a.lists_per_q = p.lists_per_q; a.work = w.work; a.done = w.done;
    a.cand_doc = w.cand_doc; a.cand_score = w.cand_score; a.cand_count = w.cand_count;
    a.doc_base = ix->d.doc_base; a.out_doc = out.doc; a.out_score = out.score; a.out_count = out.count;
    a.out_row_stride = out.row_stride; a.out_cnt_stride = out.cnt_stride;
    sl.tpu = p.tpu; sl.after_doc = after_doc; sl.after_score = after_score; sl.hint = ix->d_hint;

    SRX_TRY(ix->prof.begin(ix->opts.profile));  // profile = N: every N-th call is bracketed
    // one small memset: the worklist length and the split queries' arrival counters (a few KB: one fill launch); every other
    // slot of the workspace is initialised by the tier-1 work item that owns it
    HIP_TRY(hipMemsetAsync(w.done, 0, (size_t)(1 + (nq - p.n_whole)) * 4, stream));
    SRX_TRY(ix->prof.mark(0, stream));
    // tier 1: one wavefront per (query, split) (wave_kernel.hip)
    SRX_TRY(srx_launch_wave_kernel(sl.w, ix->d.val_type, w.items, stream));
    SRX_TRY(ix->prof.mark(1, stream));
    // tier 2 (tier2_kernel.hip): flagged units, long queries, k > 112 -- a persistent grid drains the worklist tier 1 filled.
    // Any grid size is correct; when a recent search of this index left the worklist empty (the hint word the kernel writes to
    // pinned host memory, read here without synchronisation) a small grid spares an otherwise idle launch most of its dispatch
    // time -- unless tier 1 serves nothing: full grid.
    const int hint = ix->h_hint ? *(volatile int *)ix->h_hint : -1;
    const int64_t t2_full = w.items < 1024 ? w.items : 1024;
    const bool t2_small = hint == 0 && t2_full > 128 && !tier1_serves_nothing(a.ix, k, p.tpu, a.dbg);
    const unsigned t2_grid = (unsigned)(t2_small ? 128 : t2_full);
    if (filter == nullptr)
        SRX_TRY(srx_launch_score_kernel(sl, ix->d.val_type, t2_grid, stream));
    else  // the filtered instances (tier2_filter.hip): the same descriptor plus the rows
        SRX_TRY(srx_launch_filtered_score_kernel(sl, {filter->bits, filter->q_filter, srx_filter_row_words(ix->d.n_docs)}, ix->d.val_type, t2_grid, stream));
    SRX_TRY(ix->prof.mark(2, stream));
    // merge (merge.hip): only the SPLIT queries [n_whole, nq) have lists to merge (an unsplit query's final row was written
    // by tier 1 or, when it had work for tier 2, by tier 2)
    if (nq > p.n_whole)
        SRX_TRY(srx_launch_final_merge(srx_plain_rows(w.cand_doc, w.cand_score, w.cand_count, k), nq, p.lists_per_q, k, 0, ix->d.doc_base,
                                       out, nullptr, p.n_whole, 1, (a.dbg & SRX_DBG_BLOCK_MERGE) != 0, stream));
    SRX_TRY(ix->prof.mark(3, stream));
    ix->prof.end();
    return SRX_OK;
}
}  // namespace

SRX_API int srx_search(srx_index *ix, const int32_t *q_ptr, const int32_t *q_term, const float *q_weight, int32_t nq,
                       int32_t k, int32_t *out_doc, float *out_score, int32_t *out_count, void *workspace,
                       int64_t workspace_bytes, void *stream_v) {
    return search_impl(ix, q_ptr, q_term, q_weight, nq, k, srx_plain_rows(out_doc, out_score, out_count, k), workspace,
                       workspace_bytes, stream_v);
}

SRX_API int srx_search_packed(srx_index *ix, const int32_t *q_ptr, const int32_t *q_term, const float *q_weight,
                              int32_t nq, int32_t k, int32_t *out_packed, void *workspace, int64_t workspace_bytes,
                              void *stream_v) {
    if (!out_packed || k <= 0) return fail(SRX_ERR_INVALID, "srx_search_packed: bad argument%s");
    return search_impl(ix, q_ptr, q_term, q_weight, nq, k, srx_packed_rows<float>(out_packed, k), workspace, workspace_bytes, stream_v);
}

SRX_API int srx_search_after(srx_index *ix, const int32_t *q_ptr, const int32_t *q_term, const float *q_weight, int32_t nq,
                             int32_t k, const int32_t *after_doc, const float *after_score, int32_t *out_doc, float *out_score,
                             int32_t *out_count, void *workspace, int64_t workspace_bytes, void *stream_v) {
    if (!after_doc || !after_score) return fail(SRX_ERR_INVALID, "srx_search_after: null bound arrays%s");
    return search_impl(ix, q_ptr, q_term, q_weight, nq, k, srx_plain_rows(out_doc, out_score, out_count, k), workspace,
                       workspace_bytes, stream_v, after_doc, after_score);
}

SRX_API int srx_search_after_packed(srx_index *ix, const int32_t *q_ptr, const int32_t *q_term, const float *q_weight,
                                    int32_t nq, int32_t k, const int32_t *after_doc, const float *after_score,
                                    int32_t *out_packed, void *workspace, int64_t workspace_bytes, void *stream_v) {
    if (!out_packed || k <= 0 || !after_doc || !after_score) return fail(SRX_ERR_INVALID, "srx_search_after_packed: bad argument%s");
    return search_impl(ix, q_ptr, q_term, q_weight, nq, k, srx_packed_rows<float>(out_packed, k), workspace, workspace_bytes, stream_v,
                       after_doc, after_score);
}

SRX_API int srx_search_filtered(srx_index *ix, const int32_t *q_ptr, const int32_t *q_term, const float *q_weight, int32_t nq,
                                int32_t k, const srx_doc_filter *filter, const int32_t *after_doc, const float *after_score,
                                int32_t *out_doc, float *out_score, int32_t *out_count, void *workspace, int64_t workspace_bytes,
                                void *stream_v) {
    SRX_TRY(srx_check_filter("srx_search_filtered", filter));
    return search_impl(ix, q_ptr, q_term, q_weight, nq, k, srx_plain_rows(out_doc, out_score, out_count, k), workspace,
                       workspace_bytes, stream_v, after_doc, after_score, filter);
}

SRX_API int srx_search_filtered_packed(srx_index *ix, const int32_t *q_ptr, const int32_t *q_term, const float *q_weight,
                                       int32_t nq, int32_t k, const srx_doc_filter *filter, const int32_t *after_doc,
                                       const float *after_score, int32_t *out_packed, void *workspace, int64_t workspace_bytes,
                                       void *stream_v) {
    SRX_TRY(srx_check_filter("srx_search_filtered_packed", filter));
    if (!out_packed || k <= 0) return fail(SRX_ERR_INVALID, "srx_search_filtered_packed: bad argument%s");
    return search_impl(ix, q_ptr, q_term, q_weight, nq, k, srx_packed_rows<float>(out_packed, k), workspace, workspace_bytes, stream_v,
                       after_doc, after_score, filter);
}

SRX_API int srx_profile_read(srx_index *ix, float *h_ms4) {
    if (!ix || !h_ms4) return fail(SRX_ERR_INVALID, "srx_profile_read: null argument%s");
    return ix->prof.read(h_ms4);
}

SRX_API int srx_memcpy_async(void *dst, const void *src, int64_t bytes, void *stream_v) {
    if (bytes < 0 || (bytes > 0 && (!dst || !src))) return fail(SRX_ERR_INVALID, "srx_memcpy_async: bad argument%s");
    if (bytes == 0) return SRX_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDefault, (hipStream_t)stream_v));
    return SRX_OK;
}
