// eval.hip -- ranking evaluation (eval/sparse_rx_eval.h): nDCG, AP, recall, precision, reciprocal rank, success, DCG and IDCG of
// ranked lists against graded judgments (a CSR over the judged queries), at up to 8 cutoffs per query, and their batch means.
//
// Replaces nothing in the reference project: it evaluates on the host through BEIR / pytrec_eval.
//
// The two size constants of the per-query stage:
//   SRX_EVAL_WAVE_M  = 256    m <= 256: one WAVE per query, four queries per workgroup; above: one workgroup per query.  Both are
//                             the same code over a TEAM of 64 or 256 threads, and every barrier sits at the top level, so the four
//                             waves of a workgroup meet the same barriers whatever their queries hold;
//   SRX_EVAL_LDS_ROW = 1024   a judgment row of at most 1024 (doc, grade) pairs is staged in LDS (8 KB per team) and binary-searched
//                             there; a longer row is binary-searched in global memory.  Which of the two a team takes depends on
//                             its own row only: both run inside one launch.
//
// Per-query stage, one launch, no workspace, no global atomics.  The list is taken in CHUNKS of 64 positions, one wave per chunk:
//   stage    the row goes to LDS (if it fits) while its relevant docs are counted (R); the IDCG terms gain[ideal_i] * discount[i]
//            and the ballot of "gain > 0" are written per chunk;
//   join     lane l of a chunk's wave binary-searches the doc of position 64 * chunk + l in the row; the DCG term
//            gain[g] * discount[c] and the ballots "gain > 0", "relevant", "judged" are written per chunk;
//   prefix   hits through c = the popcounts of the chunks before + the popcount of the chunk's ballot up to the lane: the AP term
//            (float)hits / (float)(c + 1) of every relevant position;
//   sums     the three ORDERED fp32 sums (DCG, IDCG, AP) of cutoff ik are taken by thread 8 * s + ik of the team, serially and in
//            ascending order below the cutoff -- the contract's order, whatever the geometry.  A chunk with few set bits in its
//            ballot is added bit by bit; a fuller one position by position (wide LDS reads, no bit scan): the terms of the
//            positions that do not contribute are stored as +0, and adding +0 to an accumulator that is never -0 changes no bit;
//   write    thread ik counts hits / judged / the first hit of its cutoff from the ballots and writes the cutoff's 8 floats and 2
//            ints.  A query that is not judged runs the same code over an empty list and an empty row: all zeros.
//
// Mean stage: srx_eval_chunk_kernel, one thread per (chunk of 1024 queries, cutoff, metric) and one per chunk for the count of
// evaluated queries, float64 sums in ascending q; srx_eval_mean_kernel, one thread per (cutoff, metric), the chunk sums in
// ascending order and ONE division.
#include "srx_common.h"
#include "eval/sparse_rx_eval.h"

#pragma clang fp contract(off)

namespace {

constexpr int EV_NK = SRX_EVAL_MAX_K;
constexpr int EV_MET = SRX_EVAL_METRICS;
constexpr int EV_CHUNK = SRX_EVAL_MEAN_CHUNK;
constexpr int EV_LOADS = 16;   // loads a thread of the mean stage keeps in flight
constexpr int EV_SPARSE = 8;   // a chunk with at most this many contributing positions is added bit by bit, a fuller one position by position
enum { EV_DCG = 0, EV_IDCG = 1, EV_AP = 2, EV_JUDGED = 3 };  // the term / ballot planes of a team

struct EvalArgs {
    const int64_t *j_ptr;       // [n_rows + 1]
    const int32_t *j_doc;       // [nnz]
    const int32_t *j_grade;     // [nnz]
    const int32_t *j_ideal;     // [nnz]
    const float *gain;          // [n_gain]
    const float *discount;      // [m]
    const int32_t *cand_doc;    // [nq][m]
    const int32_t *cand_count;  // [nq] or null
    const int32_t *q_row;       // [nq] or null
    float *out;                 // [nq][n_k][8]
    int32_t *out_hits;          // [nq][n_k]
    int32_t *out_judged;        // [nq][n_k]
    int32_t *out_rel;           // [nq]
    int64_t nnz;
    int ks[EV_NK];
    int n_rows, n_gain, rel_level, nq, m, n_k;
};

template <int MCAP>
struct EvalTeam {
    float term[3][MCAP];          // EV_DCG, EV_IDCG, EV_AP: the term of every position, +0 where it does not contribute
    uint64_t mask[4][MCAP / 64];  // the contributing positions of the three sums, and EV_JUDGED
    int32_t doc[SRX_EVAL_LDS_ROW], grade[SRX_EVAL_LDS_ROW];
    float sum[3][EV_NK];
    unsigned rel[WAVES];
};

// cutoff ik, picked by compares: a runtime index would move the argument to scratch
__device__ __forceinline__ int ev_k(const EvalArgs &a, int ik) {
    int k = a.ks[0];
#pragma unroll
    for (int j = 1; j < EV_NK; ++j)
        if (j == ik) k = a.ks[j];
    return k;
}
__device__ __forceinline__ int ev_clamp(int g, int n_gain) { return g < 0 ? 0 : g > n_gain - 1 ? n_gain - 1 : g; }
// the bits of a chunk below `r` positions (r >= 1)
__device__ __forceinline__ uint64_t ev_below(int r) { return r >= 64 ? ~0ull : (1ull << r) - 1ull; }
// is list q evaluated, and by which row
__device__ __forceinline__ int64_t ev_row(const EvalArgs &a, int64_t q) {
    const int64_t row = a.q_row != nullptr ? (int64_t)gload_i32(a.q_row + q) : q;
    return row >= 0 && row < a.n_rows ? row : -1;
}

template <int TEAM>
__global__ __launch_bounds__(THREADS) void srx_eval_kernel(EvalArgs a) {
    constexpr int MCAP = TEAM == 64 ? SRX_EVAL_WAVE_M : SRX_EVAL_MAX_M;
    constexpr int TEAMS = THREADS / TEAM, TW = TEAM / 64;
    static_assert(TEAM >= 3 * EV_NK && MCAP % 64 == 0, "a team takes the 24 ordered sums; chunks are whole");
    __shared__ EvalTeam<MCAP> s_team[TEAMS];
    const int t = threadIdx.x % TEAM, lane = t & 63, tw = t >> 6;
    EvalTeam<MCAP> &S = s_team[threadIdx.x / TEAM];
    const int64_t q = (int64_t)blockIdx.x * TEAMS + threadIdx.x / TEAM;
    const bool on = q < a.nq;  // a team past the batch runs an empty query and writes nothing: it meets every barrier
    const int m = a.m, nch = (m + 63) >> 6;  // m <= MCAP (the host picks TEAM), so 64 * nch <= MCAP

    // ---- the query: its live positions and its row [rb, rb + rlen)
    int live = 0;
    int64_t rb = 0, rlen = 0;
    if (on) {
        const int64_t row = ev_row(a, q);
        if (row >= 0) {
            live = a.cand_count != nullptr ? gload_i32(a.cand_count + q) : m;
            live = live < 0 ? 0 : live > m ? m : live;
            const int64_t b = a.j_ptr[row], e = a.j_ptr[row + 1];  // row + 1 <= n_rows: inside j_ptr
            if (b >= 0 && b <= e && e <= a.nnz) rb = b, rlen = e - b;
        }
    }
    const bool in_lds = rlen <= SRX_EVAL_LDS_ROW;
    const int nid = (int)(rlen < (int64_t)m ? rlen : (int64_t)m);

    // ---- stage
    unsigned rel = 0;
    for (int64_t i = t; i < rlen; i += TEAM) {  // rb + i < rb + rlen <= nnz
        const int g = gload_i32(a.j_grade + rb + i);
        if (in_lds) S.doc[i] = gload_i32(a.j_doc + rb + i), S.grade[i] = g;  // i < rlen <= SRX_EVAL_LDS_ROW
        rel += ev_clamp(g, a.n_gain) >= a.rel_level ? 1u : 0u;
    }
    rel = wave_sum(rel);
    if (lane == 0) S.rel[tw] = rel;
    for (int j = tw; j < nch; j += TW) {
        const int i = j * 64 + lane;  // < 64 * nch <= MCAP
        float term = 0.0f;
        bool adds = false;
        if (i < nid) {  // i < rlen and i < m: inside the row and inside discount
            const float gv = a.gain[ev_clamp(gload_i32(a.j_ideal + rb + i), a.n_gain)];
            adds = gv > 0.0f;
            term = gv * a.discount[i];
        }
        const uint64_t mk = __ballot(adds);
        S.term[EV_IDCG][i] = adds ? term : 0.0f;
        if (lane == 0) S.mask[EV_IDCG][j] = mk;
    }
    __syncthreads();

    // ---- join
    unsigned R = 0;
#pragma unroll
    for (int w = 0; w < TW; ++w) R += S.rel[w];
    for (int j = tw; j < nch; j += TW) {
        const int c = j * 64 + lane;
        float term = 0.0f;
        bool adds = false, judged = false, relevant = false;
        if (c < live) {  // c < m: inside the list and inside discount
            const int doc = gload_i32(a.cand_doc + q * m + c);
            int g = 0;
            if (in_lds) {
                int lo = 0, hi = (int)rlen;
                while (lo < hi) {  // 0 <= mid < rlen
                    const int mid = (lo + hi) >> 1;
                    if (S.doc[mid] < doc) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < (int)rlen && S.doc[lo] == doc) judged = true, g = S.grade[lo];
            } else {
                int64_t lo = 0, hi = rlen;
                while (lo < hi) {  // 0 <= mid < rlen: rb + mid < nnz
                    const int64_t mid = lo + ((hi - lo) >> 1);
                    if (gload_i32(a.j_doc + rb + mid) < doc) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < rlen && gload_i32(a.j_doc + rb + lo) == doc) judged = true, g = gload_i32(a.j_grade + rb + lo);
            }
            g = ev_clamp(g, a.n_gain);  // in [0, n_gain): inside gain
            relevant = judged && g >= a.rel_level;
            const float gv = a.gain[g];
            adds = gv > 0.0f;
            term = gv * a.discount[c];
        }
        const uint64_t m_adds = __ballot(adds), m_rel = __ballot(relevant), m_judged = __ballot(judged);
        S.term[EV_DCG][c] = adds ? term : 0.0f;
        if (lane == 0) S.mask[EV_DCG][j] = m_adds, S.mask[EV_AP][j] = m_rel, S.mask[EV_JUDGED][j] = m_judged;
    }
    __syncthreads();

    // ---- prefix
    for (int j = tw; j < nch; j += TW) {
        unsigned before = 0;
        for (int jj = 0; jj < j; ++jj) before += (unsigned)__popcll(S.mask[EV_AP][jj]);
        const uint64_t mk = S.mask[EV_AP][j];
        const int c = j * 64 + lane;
        const unsigned hits = before + (unsigned)__popcll(mk & ((2ull << lane) - 1ull));  // lane 63: 2 << 63 wraps to 0, minus 1 = all bits
        S.term[EV_AP][c] = ((mk >> lane) & 1ull) ? (float)hits / (float)(c + 1) : 0.0f;
    }
    __syncthreads();

    // ---- sums: thread 8 * s + ik takes sum s of cutoff ik
    if (t < 3 * EV_NK && (t & 7) < a.n_k) {
        const int s = t >> 3, ik = t & 7;
        const int k = ev_k(a, ik), cap = s == EV_IDCG ? nid : live;
        const int lim = k < cap ? k : cap;  // <= m
        float acc = 0.0f;
        for (int j = 0; j * 64 < lim; ++j) {  // j < nch
            const int r = lim - j * 64 < 64 ? lim - j * 64 : 64;
            const float *tp = &S.term[s][j * 64];
            uint64_t mk = S.mask[s][j] & ev_below(r);
            if (__popcll(mk) <= EV_SPARSE) {
                while (mk != 0ull) {
                    acc = acc + tp[__builtin_ctzll(mk)];
                    mk &= mk - 1ull;
                }
            } else if (r == 64) {  // the same sum: the terms in between are +0, and acc + 0 is acc (acc is never -0: it starts at +0)
#pragma unroll 16
                for (int i = 0; i < 64; ++i) acc = acc + tp[i];
            } else {
                for (int i = 0; i < r; ++i) acc = acc + tp[i];
            }
        }
        S.sum[s][ik] = acc;
    }
    __syncthreads();

    // ---- write
    if (on && t < a.n_k) {
        const int ik = t, k = ev_k(a, ik);
        const int n = k < live ? k : live;
        unsigned hits = 0, judged = 0;
        int first = -1;
        for (int j = 0; j * 64 < n; ++j) {
            const uint64_t below = ev_below(n - j * 64);
            const uint64_t r = S.mask[EV_AP][j] & below;
            if (first < 0 && r != 0ull) first = j * 64 + __builtin_ctzll(r);
            hits += (unsigned)__popcll(r);
            judged += (unsigned)__popcll(S.mask[EV_JUDGED][j] & below);
        }
        const float dcg = S.sum[EV_DCG][ik], idcg = S.sum[EV_IDCG][ik], ap = S.sum[EV_AP][ik];
        const float fr = (float)R, fh = (float)hits;
        float *o = a.out + (q * a.n_k + ik) * EV_MET;
        o[SRX_EVAL_NDCG] = idcg == 0.0f ? 0.0f : dcg / idcg;
        o[SRX_EVAL_AP] = R == 0u ? 0.0f : ap / fr;
        o[SRX_EVAL_RECALL] = R == 0u ? 0.0f : fh / fr;
        o[SRX_EVAL_P] = fh / (float)k;
        o[SRX_EVAL_RR] = first < 0 ? 0.0f : 1.0f / (float)(first + 1);
        o[SRX_EVAL_SUCCESS] = hits > 0u ? 1.0f : 0.0f;
        o[SRX_EVAL_DCG] = dcg;
        o[SRX_EVAL_IDCG] = idcg;
        a.out_hits[q * a.n_k + ik] = (int32_t)hits;
        a.out_judged[q * a.n_k + ik] = (int32_t)judged;
    }
    if (on && t == 0) a.out_rel[q] = (int32_t)R;
}

// workspace: f64 sums[n_chunks][n_k * 8], then i64 counts[n_chunks]
__global__ __launch_bounds__(THREADS) void srx_eval_chunk_kernel(EvalArgs a, double *ws_sum, int64_t *ws_cnt, int n_chunks) {
    const int per = a.n_k * EV_MET + 1;
    const int64_t idx = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (idx >= (int64_t)n_chunks * per) return;
    const int chunk = (int)(idx / per), j = (int)(idx % per);
    const int64_t q0 = (int64_t)chunk * EV_CHUNK, q1 = q0 + EV_CHUNK < a.nq ? q0 + EV_CHUNK : a.nq;
    if (j == per - 1) {
        int64_t n = 0;
        for (int64_t q = q0; q < q1; ++q) n += ev_row(a, q) >= 0 ? 1 : 0;
        ws_cnt[chunk] = n;
    } else {
        double acc = 0.0;
        for (int64_t q = q0; q < q1; q += EV_LOADS) {  // EV_LOADS loads in flight, then their adds in ascending q
            float v[EV_LOADS];
            bool ok[EV_LOADS];
#pragma unroll
            for (int u = 0; u < EV_LOADS; ++u) {
                const int64_t qq = q + u < q1 ? q + u : q1 - 1;  // inside the batch: every word of out was written by the first launch
                ok[u] = q + u < q1 && ev_row(a, qq) >= 0;
                v[u] = a.out[qq * (per - 1) + j];
            }
#pragma unroll
            for (int u = 0; u < EV_LOADS; ++u)
                if (ok[u]) acc = acc + (double)v[u];
        }
        ws_sum[(int64_t)chunk * (per - 1) + j] = acc;
    }
}

__global__ __launch_bounds__(64) void srx_eval_mean_kernel(const double *ws_sum, const int64_t *ws_cnt, int n_chunks, int n_vals, double *out_mean,
                                                           int32_t *out_n) {
    const int j = threadIdx.x;  // n_vals <= 64
    int64_t n = 0;
    for (int c = 0; c < n_chunks; ++c) n += ws_cnt[c];
    if (j < n_vals) {
        double acc = 0.0;
        for (int c = 0; c < n_chunks; ++c) acc = acc + ws_sum[(int64_t)c * n_vals + j];
        out_mean[j] = n == 0 ? 0.0 : acc / (double)n;
    }
    if (j == 0) *out_n = (int32_t)n;
}

int64_t ev_chunks(int32_t nq) { return ((int64_t)nq + EV_CHUNK - 1) / EV_CHUNK; }

}  // namespace

SRX_API int64_t srx_eval_workspace_bytes(int32_t nq, int32_t n_k) {
    if (nq < 0 || n_k < 1 || n_k > SRX_EVAL_MAX_K) return fail(SRX_ERR_INVALID, "srx_eval_workspace_bytes: need nq >= 0 and n_k in [1, 8]%s");
    return ev_chunks(nq) * ((int64_t)n_k * EV_MET * 8 + 8);
}

SRX_API int srx_eval_lists(int32_t device, const int64_t *j_ptr, const int32_t *j_doc, const int32_t *j_grade, const int32_t *j_ideal, int32_t n_rows,
                           int64_t nnz, const float *gain, int32_t n_gain, const float *discount, int32_t rel_level, const int32_t *cand_doc,
                           const int32_t *cand_count, const int32_t *q_row, int32_t nq, int32_t m, const int32_t *ks, int32_t n_k, float *out,
                           int32_t *out_hits, int32_t *out_judged, int32_t *out_rel, double *out_mean, int32_t *out_n, void *workspace,
                           int64_t workspace_bytes, void *stream_v) {
    const char *who = "srx_eval_lists";
    if (n_rows < 0 || nnz < 0) return fail(SRX_ERR_INVALID, "%s: negative n_rows / nnz", who);
    if (n_rows > 0 && (!j_ptr || !j_doc || !j_grade || !j_ideal)) return fail(SRX_ERR_INVALID, "%s: null j_ptr / j_doc / j_grade / j_ideal", who);
    if (n_gain < 1 || n_gain > SRX_EVAL_MAX_GAIN) return fail(SRX_ERR_INVALID, "%s: n_gain must be in [1, 32]", who);
    if (!gain || !discount) return fail(SRX_ERR_INVALID, "%s: null gain / discount", who);
    if (rel_level < 1) return fail(SRX_ERR_INVALID, "%s: rel_level must be >= 1", who);
    if (m < 1 || m > SRX_EVAL_MAX_M) return fail(SRX_ERR_INVALID, "%s: m must be in [1, 2048]", who);
    if (n_k < 1 || n_k > SRX_EVAL_MAX_K) return fail(SRX_ERR_INVALID, "%s: n_k must be in [1, 8]", who);
    if (!ks) return fail(SRX_ERR_INVALID, "%s: null ks", who);
    for (int i = 0; i < n_k; ++i) {
        if (ks[i] < 1) return fail(SRX_ERR_INVALID, "%s: a cutoff must be >= 1", who);
        if (i > 0 && ks[i] <= ks[i - 1]) return fail(SRX_ERR_INVALID, "%s: the cutoffs must be strictly ascending", who);
    }
    if (nq < 0 || (int64_t)nq * m > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: need nq >= 0 and nq * m <= 2^31 - 1", who);
    if ((out_mean == nullptr) != (out_n == nullptr)) return fail(SRX_ERR_INVALID, "%s: out_mean and out_n go together", who);
    const int64_t need = out_mean ? srx_eval_workspace_bytes(nq, n_k) : 0;
    if (out_mean && nq > 0 && (!workspace || ((uintptr_t)workspace & 7u) || workspace_bytes < need))
        return fail(SRX_ERR_INVALID, "%s: the means need a workspace of srx_eval_workspace_bytes, 8-byte aligned", who);
    if (nq > 0 && (!cand_doc || !out || !out_hits || !out_judged || !out_rel))
        return fail(SRX_ERR_INVALID, "%s: null cand_doc / out / out_hits / out_judged / out_rel", who);
    if (nq == 0) return SRX_OK;

    EvalArgs a;
    memset(&a, 0, sizeof(a));
    a.j_ptr = j_ptr, a.j_doc = j_doc, a.j_grade = j_grade, a.j_ideal = j_ideal, a.gain = gain, a.discount = discount;
    a.cand_doc = cand_doc, a.cand_count = cand_count, a.q_row = q_row;
    a.out = out, a.out_hits = out_hits, a.out_judged = out_judged, a.out_rel = out_rel;
    a.nnz = nnz, a.n_rows = n_rows, a.n_gain = n_gain, a.rel_level = rel_level, a.nq = nq, a.m = m, a.n_k = n_k;
    for (int i = 0; i < EV_NK; ++i) a.ks[i] = ks[i < n_k ? i : n_k - 1];

    HIP_TRY(hipSetDevice(device));
    hipStream_t stream = (hipStream_t)stream_v;
    if (m <= SRX_EVAL_WAVE_M) hipLaunchKernelGGL(srx_eval_kernel<64>, dim3((unsigned)((nq + WAVES - 1) / WAVES)), dim3(THREADS), 0, stream, a);
    else hipLaunchKernelGGL(srx_eval_kernel<THREADS>, dim3((unsigned)nq), dim3(THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    if (out_mean) {
        const int n_chunks = (int)ev_chunks(nq), n_vals = n_k * EV_MET;
        double *ws_sum = (double *)workspace;
        int64_t *ws_cnt = (int64_t *)(ws_sum + (int64_t)n_chunks * n_vals);
        const int64_t threads = (int64_t)n_chunks * (n_vals + 1);
        hipLaunchKernelGGL(srx_eval_chunk_kernel, dim3((unsigned)((threads + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream, a, ws_sum, ws_cnt, n_chunks);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(srx_eval_mean_kernel, dim3(1), dim3(64), 0, stream, ws_sum, ws_cnt, n_chunks, n_vals, out_mean, out_n);
        HIP_TRY(hipGetLastError());
    }
    return SRX_OK;
}
