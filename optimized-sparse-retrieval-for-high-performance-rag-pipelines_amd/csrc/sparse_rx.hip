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

thread_local char srx_g_err[512] = "";

constexpr int PROF_SLOTS = 256;
constexpr int PROF_EVENTS = 4;  // start, after tier 1, after tier 2, after merge
struct srx_index {
    srx_index_desc d;
    srx_search_opts opts;
    hipEvent_t *ev;   // PROF_SLOTS x PROF_EVENTS events, created lazily
    int ev_n;         // profiled calls recorded since the last srx_profile_read (<= PROF_SLOTS, then it wraps)
    int64_t ev_calls;
    int64_t n_calls;  // searches issued (profile = N samples every N-th of them)
    int *h_hint;      // pinned, device-mapped word: the tier-2 worklist length of a recent search (sizes the next tier-2 grid)
    int *d_hint;      // its device address
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
    srx_index *ix = new (std::nothrow) srx_index();
    if (!ix) return fail(SRX_ERR_NOMEM, "srx_index_create: host allocation failed%s");
    ix->d = *d;
    memset(&ix->opts, 0, sizeof(ix->opts));
    ix->ev = nullptr;
    ix->ev_n = 0;
    ix->ev_calls = 0;
    ix->n_calls = 0;
    // 64 bytes of pinned host memory, created once with the handle (srx_search itself allocates nothing).  Not fatal when
    // it cannot be had: the tier-2 grid then always has its full size.
    ix->h_hint = nullptr;
    ix->d_hint = nullptr;
    if (hipSetDevice(d->device) == hipSuccess && hipHostMalloc((void **)&ix->h_hint, 64, hipHostMallocMapped) == hipSuccess) {
        ix->h_hint[0] = -1;  // unknown
        if (hipHostGetDevicePointer((void **)&ix->d_hint, ix->h_hint, 0) != hipSuccess) {
            (void)hipHostFree(ix->h_hint);
            ix->h_hint = nullptr;
            ix->d_hint = nullptr;
        }
    } else {
        ix->h_hint = nullptr;
        (void)hipGetLastError();
    }
    *out = ix;
    return SRX_OK;
}

SRX_API void srx_index_destroy(srx_index *ix) {
    if (!ix) return;
    if (ix->ev) {
        for (int i = 0; i < PROF_EVENTS * PROF_SLOTS; ++i) (void)hipEventDestroy(ix->ev[i]);
        delete[] ix->ev;
    }
    if (ix->h_hint) (void)hipHostFree(ix->h_hint);
    delete ix;
}

SRX_API int srx_index_set_opts(srx_index *ix, const srx_search_opts *o) {
    if (!ix || !o) return fail(SRX_ERR_INVALID, "srx_index_set_opts: null argument%s");
    if (o->supertile_log2 != 0 && (o->supertile_log2 < ix->d.tile_log2 || o->supertile_log2 > ix->d.tile_log2 + 6))
        return fail(SRX_ERR_INVALID, "srx_index_set_opts: supertile_log2 must be in [tile_log2, tile_log2+6]%s");
    if (o->unit_tiles < 0 || o->unit_tiles > MAX_TPS) return fail(SRX_ERR_INVALID, "srx_index_set_opts: unit_tiles must be in [0, 64]%s");
    if (o->target_blocks < 0) return fail(SRX_ERR_INVALID, "srx_index_set_opts: target_blocks < 0%s");
    if (o->reserved & ~(8 | 16 | 128 | 256 | 2048 | 4096 | 8192))
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
int search_impl(srx_index *ix, const int32_t *q_ptr, const int32_t *q_term, const float *q_weight, int32_t nq,
                int32_t k, const srx_rows &out, void *workspace, int64_t workspace_bytes, void *stream_v,
                const int32_t *after_doc = nullptr, const float *after_score = nullptr) {
    if (!ix) return fail(SRX_ERR_INVALID, "srx_search: null index%s");
    if ((after_doc == nullptr) != (after_score == nullptr)) return fail(SRX_ERR_INVALID, "srx_search_after: after_doc and after_score go together%s");
    if (nq < 0 || k <= 0 || k > KMAX) return fail(SRX_ERR_INVALID, "srx_search: need nq >= 0 and 1 <= k <= 1024%s");
    if (nq == 0) return SRX_OK;
    if (!q_ptr || !out.doc || !out.score || !out.count) return fail(SRX_ERR_INVALID, "srx_search: null query / output pointer%s");
    const Plan p = make_plan(ix, nq, k);
    const SearchWs w = search_ws(workspace, p, nq, k);
    if (!workspace || workspace_bytes < w.bytes) return fail(SRX_ERR_NOMEM, "srx_search: workspace too small%s");
    hipStream_t stream = (hipStream_t)stream_v;
    HIP_TRY(hipSetDevice(ix->d.device));
    if (ix->d.post == nullptr && p.tpu != ix->d.unit_tiles)
        return fail(SRX_ERR_INVALID, "srx_search: this index keeps no canonical blocks: a unit other than the one it was built for cannot be served%s");
    const int64_t blocks = w.items;  // work items: one per unsplit query, n_splits per split query
    if (w.lists > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "srx_search: nq * splits overflows the grid%s");

    IndexView v;
    v.term_ptr = ix->d.term_ptr;
    v.post = ix->d.post;
    v.post16 = ix->d.post16;
    v.zero_block = ix->d.n_blocks;
    v.unit_tiles = ix->d.unit_tiles;
    v.tile_skip = ix->d.tile_skip;
    v.idf = ix->d.idf;
    v.term_bound = ((ix->opts.reserved & 16) || after_score) ? nullptr : ix->d.term_bound;  // debug bit 16: ignore the score bounds
    v.n_docs = ix->d.n_docs;
    v.vocab = ix->d.vocab;
    v.tile_log2 = ix->d.tile_log2;
    v.n_tiles = ix->d.n_tiles;
    const int dbg = ix->opts.reserved | (after_score ? 8 : 0);  // search-after: the tier-2 kernel applies the bound, it takes every query

    const bool prof = ix->opts.profile > 0 && (ix->n_calls++ % ix->opts.profile) == 0;  // profile = N: every N-th call is bracketed
    hipEvent_t *ev = nullptr;
    if (prof) {
        if (!ix->ev) {
            ix->ev = new (std::nothrow) hipEvent_t[PROF_EVENTS * PROF_SLOTS];
            if (!ix->ev) return fail(SRX_ERR_NOMEM, "srx_search: host allocation failed%s");
            for (int i = 0; i < PROF_EVENTS * PROF_SLOTS; ++i) HIP_TRY(hipEventCreate(&ix->ev[i]));
        }
        ev = ix->ev + PROF_EVENTS * (int)(ix->ev_calls % PROF_SLOTS);
    }
    // one small memset: the worklist length and the split queries' arrival counters (a few KB: one fill launch); every other
    // slot of the workspace is initialised by the tier-1 work item that owns it
    HIP_TRY(hipMemsetAsync(w.done, 0, (size_t)(1 + (nq - p.n_whole)) * 4, stream));
    if (prof) HIP_TRY(hipEventRecord(ev[0], stream));
    // tier 1: one wavefront per (query, split) (wave_kernel.hip)
    {
        srx_wave_launch wl;
        wl.ix = v;
        wl.q_ptr = q_ptr; wl.q_term = q_term; wl.q_weight = q_weight;
        wl.nq = nq; wl.k = k; wl.n_splits = p.n_splits; wl.n_whole = p.n_whole; wl.n_super = p.n_super;
        wl.dbg = dbg | (p.tpu != ix->d.unit_tiles ? 8 : 0);  // another unit than the padded one: everything to tier 2
        wl.ovf = w.ovf; wl.ovf_words = p.ovf_words; wl.lists_per_q = p.lists_per_q; wl.work = w.work; wl.done = w.done;
        wl.cand_doc = w.cand_doc; wl.cand_score = w.cand_score; wl.cand_count = w.cand_count;
        wl.doc_base = ix->d.doc_base; wl.out_doc = out.doc; wl.out_score = out.score; wl.out_count = out.count;
        wl.out_row_stride = out.row_stride; wl.out_cnt_stride = out.cnt_stride;
        const int rc = srx_launch_wave_kernel(wl, ix->d.val_type, blocks, stream);
        if (rc != SRX_OK) return rc;
    }
    if (prof) HIP_TRY(hipEventRecord(ev[1], stream));
    // tier 2 (tier2_kernel.hip): flagged units, long queries, k > 112 -- a persistent grid drains the worklist tier 1 filled.
    // Any grid size is correct; when a recent search of this index left the worklist empty (the hint word the kernel writes to
    // pinned host memory, read here without synchronisation) a small grid spares an otherwise idle launch most of its dispatch
    // time.
    {
        const int dbg2 = dbg | (p.tpu != ix->d.unit_tiles ? 8 : 0);
        const bool t2_everything = (dbg2 & 8) != 0 || k > W1_KMAX || ix->d.post16 == nullptr;  // tier 1 serves nothing: full grid
        const int hint = ix->h_hint ? *(volatile int *)ix->h_hint : -1;
        const int64_t t2_full = blocks < 1024 ? blocks : 1024;
        const unsigned t2_grid = (unsigned)((hint == 0 && !t2_everything && t2_full > 128) ? 128 : t2_full);
        srx_score_launch sl;
        sl.ix = v;
        sl.q_ptr = q_ptr; sl.q_term = q_term; sl.q_weight = q_weight;
        sl.nq = nq; sl.k = k; sl.n_splits = p.n_splits; sl.n_whole = p.n_whole; sl.tpu = p.tpu; sl.n_super = p.n_super;
        sl.dbg = dbg2;
        sl.ovf = w.ovf; sl.ovf_words = p.ovf_words; sl.lists_per_q = p.lists_per_q; sl.work = w.work;
        sl.cand_doc = w.cand_doc; sl.cand_score = w.cand_score; sl.cand_count = w.cand_count;
        sl.after_doc = after_doc; sl.after_score = after_score;
        sl.doc_base = ix->d.doc_base; sl.out_doc = out.doc; sl.out_score = out.score; sl.out_count = out.count;
        sl.out_row_stride = out.row_stride; sl.out_cnt_stride = out.cnt_stride; sl.hint = ix->d_hint;
        const int rc = srx_launch_score_kernel(sl, ix->d.val_type, t2_grid, stream);
        if (rc != SRX_OK) return rc;
    }
    if (prof) HIP_TRY(hipEventRecord(ev[2], stream));
    // merge (merge.hip): only the SPLIT queries [n_whole, nq) have lists to merge (an unsplit query's final row was written
    // by tier 1 or, when it had work for tier 2, by tier 2); debug bit 256 forces the block kernel
    if (nq > p.n_whole) {
        const int rc = srx_launch_final_merge(srx_plain_rows(w.cand_doc, w.cand_score, w.cand_count, k), nq, p.lists_per_q, k, 0,
                                              ix->d.doc_base, out, nullptr, p.n_whole, 1, (dbg & 256) != 0, stream);
        if (rc != SRX_OK) return rc;
    }
    if (prof) {
        HIP_TRY(hipEventRecord(ev[3], stream));
        ++ix->ev_calls;
        if (ix->ev_n < PROF_SLOTS) ++ix->ev_n;
    }
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

SRX_API int srx_profile_read(srx_index *ix, float *h_ms4) {
    if (!ix || !h_ms4) return fail(SRX_ERR_INVALID, "srx_profile_read: null argument%s");
    if (ix->ev_n == 0 || !ix->ev) return fail(SRX_ERR_INVALID, "srx_profile_read: no profiled srx_search has run%s");
    double acc[4] = {0, 0, 0, 0};
    for (int i = 0; i < ix->ev_n; ++i) {
        const int slot = (int)((ix->ev_calls - 1 - i) % PROF_SLOTS);
        hipEvent_t *ev = ix->ev + PROF_EVENTS * slot;
        float a = 0, b = 0, c = 0, d = 0;
        HIP_TRY(hipEventSynchronize(ev[3]));
        HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
        HIP_TRY(hipEventElapsedTime(&b, ev[1], ev[2]));
        HIP_TRY(hipEventElapsedTime(&c, ev[2], ev[3]));
        HIP_TRY(hipEventElapsedTime(&d, ev[0], ev[3]));
        acc[0] += a;
        acc[1] += b;
        acc[2] += c;
        acc[3] += d;
    }
    for (int j = 0; j < 4; ++j) h_ms4[j] = (float)(acc[j] / ix->ev_n);
    const int n = ix->ev_n;
    ix->ev_n = 0;
    return n;
}

SRX_API int srx_memcpy_async(void *dst, const void *src, int64_t bytes, void *stream_v) {
    if (bytes < 0 || (bytes > 0 && (!dst || !src))) return fail(SRX_ERR_INVALID, "srx_memcpy_async: bad argument%s");
    if (bytes == 0) return SRX_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, hipMemcpyDefault, (hipStream_t)stream_v));
    return SRX_OK;
}
