// terms.hip -- term constraints (sparse_rx_terms.h): filter rows built from the posting lists.  Row r allows doc d iff the base
// row allows it, d has every term of all[r], one term of any[r] (when the list is not empty) and no term of none[r].
//
// Replaces nothing in the reference project: it has no filters.
//
// One workgroup per (chunk of docs, output row).  A chunk is the index's unit (unit_tiles << tile_log2 <= 49152 docs) wherever a
// unit fits the LDS bitmaps -- always, when the compact copy is read --, else the most tiles of the canonical copy that do.  It
// is a multiple of 64 docs (tile_log2 >= 6), so it starts on a word boundary of the row.  Two LDS bitmaps of the chunk:
//     acc   starts as the base row's words (or all ones), tail bits at or above n_docs and the row's padding words cleared;
//     tmp   the docs of the chunk that have a term (or one of a list's terms): cleared, then a DS OR per posting.
// all:  per term, tmp = its docs, acc &= tmp.  any: tmp = the docs of every term, acc &= tmp.  none: the same, acc &= ~tmp.
// The workgroup stops folding once acc is all zero and stores what it has; every word of its slice of the row is stored.
//
// The run of term t in the chunk of tiles [j0, j1) is [term_ptr[t] + tile_skip[t][j0], term_ptr[t] + tile_skip[t][j1]): block
// aligned where the chunk is a unit (srx_common.h).  A thread takes one block of 4 postings per step and ORs them into tmp, ids
// that share a word as one mask (ids ascend inside a run, so they mostly do).  An id is used iff its chunk-local value is below
// the chunk's doc count: that drops the sentinels of both copies (negative ids; local ids >= 49152) before the LDS atomic --
// many lanes on one dummy address would serialise -- and, where a chunk is not a unit, the neighbouring tiles' postings of the
// first and last block.  Values are never read: the value type only sets the block stride.
//
// A term id outside [0, vocab) is read as "no doc has it" (-1 is the legal spelling; any other is a precondition violation that
// the kernel does not turn into a wild read).
#include "desc_check.h"
#include "filter_common.h"
#include "sparse_rx_terms.h"

namespace {

constexpr int TM_WORDS = W_UNIT_MAX_DOCS / 32 + 4;  // a chunk's words, plus the <= 3 padding words of a row that ends in it
constexpr int TM_MAX_ROWS_Y = 65535;                // grid.y; more rows than that are looped over

struct TermsArgs {
    const int64_t *term_ptr;
    const int32_t *post;  // the copy the instance reads: canonical blocks, or the compact copy
    const int32_t *tile_skip;
    const int32_t *lptr[3], *lterm[3];  // all, any, none
    const uint32_t *base_bits;          // null: every doc
    const int32_t *base_q;              // null: base row 0
    uint32_t *out;
    int64_t n_docs, vocab, words;
    int n_rows, n_tiles, tile_log2, chunk_tiles, n_chunks;
};

struct Chunk {
    int j0, j1;       // its tiles
    unsigned first;   // its first doc
    unsigned docs;    // docs it spans (a multiple of 64; the last chunk's tail lies beyond n_docs)
};

// tmp |= the docs of the chunk that have term t
template <int STRIDE, bool COMPACT>
__device__ __forceinline__ void scatter_term(const TermsArgs &a, int t, const Chunk &c, uint32_t *tmp) {
    const int32_t *sk = a.tile_skip + (int64_t)t * ((int64_t)a.n_tiles + 1);
    const unsigned s0 = (unsigned)cload_i32(sk + c.j0), s1 = (unsigned)cload_i32(sk + c.j1);
    const int32_t *blk0 = a.post + ((cload_i64(a.term_ptr + t) >> 2) + (int64_t)(s0 >> 2)) * STRIDE;
    const unsigned nb = ((s1 + 3u) >> 2) - (s0 >> 2);  // s0 <= s1
    for (unsigned b = threadIdx.x; b < nb; b += THREADS) {
        const int32_t *blk = blk0 + (size_t)b * STRIDE;
        unsigned l[4];
        if constexpr (COMPACT) {
            const srx_i2u w = gload_i2(blk);
            l[0] = (unsigned)w.x & 0xFFFFu; l[1] = (unsigned)w.x >> 16;
            l[2] = (unsigned)w.y & 0xFFFFu; l[3] = (unsigned)w.y >> 16;
        } else {
            const srx_i4u w = gload_i4(blk);
            l[0] = (unsigned)w.x - c.first; l[1] = (unsigned)w.y - c.first;
            l[2] = (unsigned)w.z - c.first; l[3] = (unsigned)w.w - c.first;
        }
        unsigned cur = 0u, mask = 0u;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
            if (l[n] >= c.docs) continue;  // a sentinel, or a posting of a neighbouring chunk
            const unsigned w = l[n] >> 5, m = 1u << (l[n] & 31u);
            if (mask != 0u && w != cur) {
                atomicOr(&tmp[cur], mask);
                mask = 0u;
            }
            cur = w;
            mask |= m;
        }
        if (mask != 0u) atomicOr(&tmp[cur], mask);
    }
}

template <int STRIDE, bool COMPACT>
__global__ __launch_bounds__(THREADS) void srx_terms_kernel(TermsArgs a) {
    __shared__ uint32_t acc[TM_WORDS], tmp[TM_WORDS];
    const int tid = threadIdx.x, u = blockIdx.x;
    Chunk c;
    c.j0 = u * a.chunk_tiles;
    c.j1 = min(c.j0 + a.chunk_tiles, a.n_tiles);
    c.first = (unsigned)c.j0 << a.tile_log2;
    c.docs = (unsigned)a.chunk_tiles << a.tile_log2;
    const int cw = (int)(c.docs >> 5);
    const int64_t w0 = (int64_t)u * cw;                                 // the chunk's first word of a row
    const int nw = u == a.n_chunks - 1 ? (int)(a.words - w0) : cw;      // the last chunk also owns the padding words: <= cw + 3
    for (int r = blockIdx.y; r < a.n_rows; r += gridDim.y) {
        const int br = srx_filter_base_row(a.base_bits, a.base_q, r);
        const uint32_t *brow = br >= 0 ? a.base_bits + (int64_t)br * a.words + w0 : nullptr;
        // word w of acc / tmp belongs to thread w % THREADS until the store
        for (int w = tid; w < nw; w += THREADS) {
            const int64_t left = a.n_docs - (w0 + w) * 32;  // docs from the word's first bit on
            const uint32_t valid = left >= 32 ? 0xFFFFFFFFu : left > 0 ? (1u << (int)left) - 1u : 0u;
            acc[w] = brow != nullptr ? brow[w] & valid : valid;
        }
        bool live = true;  // uniform: acc may still hold a bit
        // ---- all: one pass per term
        if (a.lptr[0] != nullptr) {
            const int p0 = cload_i32(a.lptr[0] + r), p1 = cload_i32(a.lptr[0] + r + 1);
            for (int i = p0; i < p1 && live; ++i) {
                const int t = cload_i32(a.lterm[0] + i);
                const bool known = t >= 0 && (int64_t)t < a.vocab;
                for (int w = tid; w < nw; w += THREADS) tmp[w] = 0u;
                __syncthreads();
                if (known) scatter_term<STRIDE, COMPACT>(a, t, c, tmp);
                __syncthreads();
                uint32_t nz = 0u;
                for (int w = tid; w < nw; w += THREADS) {
                    const uint32_t x = acc[w] & tmp[w];
                    acc[w] = x;
                    nz |= x;
                }
                live = __syncthreads_or(nz != 0u) != 0;
            }
        }
        // ---- any, then none: one pass per list
#pragma unroll
        for (int which = 1; which <= 2; ++which) {
            if (a.lptr[which] == nullptr || !live) continue;
            const int p0 = cload_i32(a.lptr[which] + r), p1 = cload_i32(a.lptr[which] + r + 1);
            if (p1 <= p0) continue;
            for (int w = tid; w < nw; w += THREADS) tmp[w] = 0u;
            __syncthreads();
            for (int i = p0; i < p1; ++i) {
                const int t = cload_i32(a.lterm[which] + i);
                if (t >= 0 && (int64_t)t < a.vocab) scatter_term<STRIDE, COMPACT>(a, t, c, tmp);
            }
            __syncthreads();
            uint32_t nz = 0u;
            for (int w = tid; w < nw; w += THREADS) {
                const uint32_t x = acc[w] & (which == 1 ? tmp[w] : ~tmp[w]);
                acc[w] = x;
                nz |= x;
            }
            live = __syncthreads_or(nz != 0u) != 0;
        }
        __syncthreads();  // acc is complete for every thread
        uint32_t *orow = a.out + (int64_t)r * a.words + w0;
        if ((cw & 3) == 0) {  // w0 and nw are multiples of 4: 16-byte stores
            for (int w = tid * 4; w < nw; w += THREADS * 4)
                *reinterpret_cast<uint4 *>(orow + w) = make_uint4(acc[w], acc[w + 1], acc[w + 2], acc[w + 3]);
        } else {
            for (int w = tid; w < nw; w += THREADS) orow[w] = acc[w];
        }
        __syncthreads();  // before the next row's acc
    }
}

template <int STRIDE, bool COMPACT>
int launch_terms(const TermsArgs &a, hipStream_t stream) {
    const unsigned gy = (unsigned)(a.n_rows < TM_MAX_ROWS_Y ? a.n_rows : TM_MAX_ROWS_Y);
    hipLaunchKernelGGL((srx_terms_kernel<STRIDE, COMPACT>), dim3((unsigned)a.n_chunks, gy), dim3(THREADS), 0, stream, a);
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

}  // namespace

SRX_API int64_t srx_filter_from_terms_bytes(int64_t n_rows, int64_t n_docs) {
    if (n_rows < 0 || n_docs < 1 || n_docs > SRX_FILTER_MAX_DOCS)
        return fail(SRX_ERR_INVALID, "srx_filter_from_terms_bytes: need n_rows >= 0 and n_docs in [1, 2^31 - 2]%s");
    const int64_t row_bytes = srx_filter_row_words(n_docs) * 4;
    if (n_rows > INT64_MAX / row_bytes) return fail(SRX_ERR_INVALID, "srx_filter_from_terms_bytes: the size does not fit int64%s");
    return n_rows * row_bytes;
}

SRX_API int srx_filter_from_terms(const srx_index_desc *d, int32_t n_rows, const int32_t *all_ptr, const int32_t *all_term,
                                  const int32_t *any_ptr, const int32_t *any_term, const int32_t *none_ptr, const int32_t *none_term,
                                  const srx_doc_filter *base, uint32_t *out_bits, void *stream_v) {
    const char *who = "srx_filter_from_terms";
    int rc = srx_check_index_desc(who, d);
    if (rc == SRX_OK) rc = srx_check_row_builder(who, "term", n_rows, all_ptr, all_term, any_ptr, any_term, none_ptr, none_term, out_bits, base);
    if (rc != SRX_OK) return rc;
    if (n_rows == 0) return SRX_OK;
    HIP_TRY(hipSetDevice(d->device));
    const bool compact = d->post16 != nullptr;
    TermsArgs a;
    a.term_ptr = d->term_ptr;
    a.post = compact ? d->post16 : d->post;
    a.tile_skip = d->tile_skip;
    a.lptr[0] = all_ptr, a.lterm[0] = all_term;
    a.lptr[1] = any_ptr, a.lterm[1] = any_term;
    a.lptr[2] = none_ptr, a.lterm[2] = none_term;
    a.base_bits = base ? base->bits : nullptr;
    a.base_q = base ? base->q_filter : nullptr;
    a.out = out_bits;
    a.n_docs = d->n_docs;
    a.vocab = d->vocab;
    a.words = srx_filter_row_words(d->n_docs);
    a.n_rows = n_rows;
    a.n_tiles = d->n_tiles;
    a.tile_log2 = d->tile_log2;
    const bool unit_fits = ((int64_t)d->unit_tiles << d->tile_log2) <= W_UNIT_MAX_DOCS;
    a.chunk_tiles = unit_fits ? d->unit_tiles : W_UNIT_MAX_DOCS >> d->tile_log2;  // the canonical copy in units too large for the bitmaps
    a.n_chunks = (d->n_tiles + a.chunk_tiles - 1) / a.chunk_tiles;
    hipStream_t stream = (hipStream_t)stream_v;
    if (d->val_type == SRX_VAL_F32)
        return compact ? launch_terms<CompactWords<float>::value, true>(a, stream) : launch_terms<BlockWords<float>::value, false>(a, stream);
    return compact ? launch_terms<CompactWords<__half>::value, true>(a, stream) : launch_terms<BlockWords<__half>::value, false>(a, stream);
}
