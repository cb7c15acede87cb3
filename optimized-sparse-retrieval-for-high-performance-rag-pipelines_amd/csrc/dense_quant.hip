// dense_quant.hip -- the dense index build and the per-search query quantisation on the device (srx_dense_quantize_i8 / _u8,
// srx_dense_quantize_queries_i8 / _u8; include/sparse_rx_quant.h): the reference's _quantize_embeddings and query
// quantisers (rag_system/core/retriever_registry.py:435-462, 482-491, 555) operation by operation in fp32.  Same build flags
// as the other units; -ffp-contract=off is the contract (every multiply, add and IEEE divide rounded on its own).
//
// A streaming pass bound by HBM: 4 bytes read and 1 written per element.  One workgroup = one tile of 32 rows (the tile of
// the fragment order srx_dense_pack_i8 documents), one wave = 8 of them, a row at a time:
//   load      lane l holds columns 4 l + 256 j + (0 .. 3), j < NJ, of its row: one coalesced 16-byte load per j when the
//             base is 16-byte aligned and ld and dim are multiples of 4 (uniform per launch), else four 4-byte loads.  DQ_U
//             rows are loaded before the first is used.  The row stays in registers: it is read once.
//   extrema   max |x| (i8) or min and max (u8) over the lane's elements, then an xor butterfly over the wave: no LDS.
//   codes     the row's expression per element; four codes make one word.  The words go to the tile's image in LDS
//             (row pitch NJ * 256 + 16 bytes: 16-byte reads down a column of 32 rows hit different banks).
//   store     after one barrier the workgroup writes the tile with 16-byte stores: row-major it is one contiguous block of
//             32 * dim_pad bytes; in fragment order a wave-level store is the contiguous KiB of one (tile, k-step).
//   scales    lane 0 writes the row's scale (and minimum); the de-quantised uint8 query goes out from registers as float4.
// No float atomics, no scratch, no workspace.  The flag word takes one integer atomic OR per wave that saw a flagged row.
#include "srx_common.h"
#include "sparse_rx_quant.h"

namespace {

typedef int dq_v4i __attribute__((ext_vector_type(4)));
typedef float dq_v4f __attribute__((ext_vector_type(4)));
constexpr int DQ_TILE = 32;               // rows per workgroup
constexpr int DQ_ROWS = DQ_TILE / WAVES;  // rows per wave
constexpr int DQ_U = 4;                   // rows a wave has in flight

enum DqMode { DQ_I8_ROW = 0, DQ_I8_QUERY = 1, DQ_U8_ROW = 2, DQ_U8_QUERY = 3 };

struct DenseQuantArgs {
    const float *in;          // the chunk's rows (row stride ld elements)
    int64_t ld, n_rows;       // rows of this call
    int64_t row0, n_total;    // where they sit in the whole corpus (queries: 0, nq)
    int dim, dim_pad, packed;
    void *out_codes;          // i8 / u8 codes of the WHOLE corpus (u8 query: may be null)
    float *out_scale;         // i8: f32[n_total]; u8 row: f32[2 n_total]; u8 query: f32[nq][2] (may be null)
    float *out_deq;           // u8 query only
    int32_t *flag;            // may be null
};

__device__ __forceinline__ float dq_wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float dq_wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ bool dq_nonfinite(float v) { return (__float_as_uint(v) & 0x7F800000u) == 0x7F800000u; }

template <int NJ, bool VEC, int MODE>
__global__ __launch_bounds__(THREADS) void srx_dense_quant_kernel(DenseQuantArgs a) {
    constexpr bool IS_U8 = MODE == DQ_U8_ROW || MODE == DQ_U8_QUERY;
    constexpr bool IS_QUERY = MODE == DQ_I8_QUERY || MODE == DQ_U8_QUERY;
    constexpr int PITCH = NJ * 256 + 16;  // bytes between two rows of the tile image
    __shared__ __attribute__((aligned(16))) unsigned char tile[DQ_TILE * PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t t0 = (int64_t)blockIdx.x * DQ_TILE;                // the tile's first row, relative to row0
    const int live = (int)min((int64_t)DQ_TILE, a.n_rows - t0);      // rows of the tile this call holds (>= 1)
    const bool want_codes = a.out_codes != nullptr;                  // uniform
    int flagbits = 0;                                                // wave-uniform

    for (int g = 0; g < DQ_ROWS; g += DQ_U) {
        float x[DQ_U][NJ][4];
#pragma unroll
        for (int u = 0; u < DQ_U; ++u) {
            const int r = wave * DQ_ROWS + g + u;
            const float *row = a.in + (t0 + r) * a.ld;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int c = 4 * lane + 256 * j;
                if constexpr (VEC) {  // dim % 4 == 0: the four columns are inside the row together
                    dq_v4f v = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (r < live && c < a.dim) v = *reinterpret_cast<const dq_v4f *>(row + c);
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[u][j][e] = v[e];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[u][j][e] = (r < live && c + e < a.dim) ? row[c + e] : 0.0f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < DQ_U; ++u) {
            const int r = wave * DQ_ROWS + g + u;
            unsigned *trow = reinterpret_cast<unsigned *>(tile + r * PITCH);
            if (r >= live) {  // uniform: a row the call does not hold; the fragment order stores it as zeros
                if (want_codes) {
#pragma unroll
                    for (int j = 0; j < NJ; ++j) trow[lane + 64 * j] = 0u;
                }
                continue;
            }
            // ---- extrema (the columns beyond dim hold +0: harmless for max |x|, masked for min / max) ----
            bool bad = false;
            float lo = INFINITY, hi = IS_U8 ? -INFINITY : 0.0f;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = x[u][j][e];
                    bad = bad || dq_nonfinite(v);
                    if constexpr (IS_U8) {
                        if (4 * lane + 256 * j + e < a.dim) {
                            lo = fminf(lo, v);
                            hi = fmaxf(hi, v);
                        }
                    } else {
                        hi = fmaxf(hi, fabsf(v));
                    }
                }
            bad = __ballot(bad) != 0ull;
            hi = dq_wave_max(hi);
            if constexpr (IS_U8) lo = dq_wave_min(lo);
            // ---- the row's scale (and minimum); zero = every code is 0 ----
            float s, mn = 0.0f, stored;
            bool zero = false;
            if constexpr (IS_U8) {
                const float d = hi - lo;
                bad = bad || dq_nonfinite(d);
                s = d / 255.0f;
                mn = lo;
                if constexpr (!IS_QUERY) s = fmaxf(s, 1e-8f);
                if (bad) {
                    s = IS_QUERY ? 0.0f : 1e-8f;
                    mn = 0.0f;
                    zero = true;
                    flagbits |= SRX_QUANT_NONFINITE;
                } else if (IS_QUERY && s == 0.0f) {
                    zero = true;
                    flagbits |= SRX_QUANT_DEGENERATE;
                }
                stored = s;
            } else {
                s = IS_QUERY ? hi : fmaxf(hi, 1e-8f);
                stored = IS_QUERY ? s / 127.0f : s;
                if (bad) {
                    stored = IS_QUERY ? 0.0f : 1e-8f;
                    zero = true;
                    flagbits |= SRX_QUANT_NONFINITE;
                } else if (IS_QUERY && s == 0.0f) {
                    stored = 0.0f;
                    zero = true;
                    flagbits |= SRX_QUANT_DEGENERATE;
                }
            }
            const int64_t grow = a.row0 + t0 + r;
            if (lane == 0 && a.out_scale != nullptr) {
                if constexpr (MODE == DQ_U8_ROW) {
                    a.out_scale[grow] = stored;
                    a.out_scale[a.n_total + grow] = mn;
                } else if constexpr (MODE == DQ_U8_QUERY) {
                    a.out_scale[2 * grow] = stored;
                    a.out_scale[2 * grow + 1] = mn;
                } else {
                    a.out_scale[grow] = stored;
                }
            }
            // ---- codes ----
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                unsigned word = 0u;
                dq_v4f deq = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = x[u][j][e];
                    int code = IS_U8 ? (int)rintf((v - mn) / s) : (int)rintf((v / s) * 127.0f);
                    const bool pad = 4 * lane + 256 * j + e >= a.dim;
                    if (zero || pad) code = 0;
                    word |= ((unsigned)code & 0xFFu) << (8 * e);
                    if constexpr (MODE == DQ_U8_QUERY) deq[e] = pad ? 0.0f : (float)code * s + mn;
                }
                if (want_codes) trow[lane + 64 * j] = word;
                if constexpr (MODE == DQ_U8_QUERY) {
                    const int c = 4 * lane + 256 * j;
                    if (c < a.dim_pad) *reinterpret_cast<dq_v4f *>(a.out_deq + grow * a.dim_pad + c) = deq;
                }
            }
        }
    }
    if (flagbits != 0 && lane == 0 && a.flag != nullptr) atomicOr(a.flag, flagbits);

    if (want_codes) {  // uniform
        __syncthreads();
        dq_v4i *out = reinterpret_cast<dq_v4i *>(a.out_codes);
        if (a.packed) {  // unit i of the tile: k-step i >> 6, lane i & 63 = row (i & 31), half (i >> 5) & 1
            const int units = 2 * a.dim_pad;  // 16-byte units of a whole tile
            const int64_t base = ((a.row0 >> 5) + blockIdx.x) * (int64_t)units;
            for (int i = threadIdx.x; i < units; i += THREADS) {
                const int ln = i & 63;
                out[base + i] = *reinterpret_cast<const dq_v4i *>(tile + (ln & 31) * PITCH + 32 * (i >> 6) + 16 * (ln >> 5));
            }
        } else {
            const int upr = a.dim_pad >> 4;  // units per row
            const int64_t base = (a.row0 + t0) * upr;
            for (int i = threadIdx.x; i < live * upr; i += THREADS) {
                const int r = i / upr;
                out[base + i] = *reinterpret_cast<const dq_v4i *>(tile + r * PITCH + 16 * (i - r * upr));
            }
        }
    }
}

template <int MODE>
void dq_launch(const DenseQuantArgs &a, bool vec, hipStream_t stream) {
    const unsigned blocks = (unsigned)((a.n_rows + DQ_TILE - 1) / DQ_TILE);
    const int nj = (a.dim_pad + 255) / 256;
#define SRX_DQ(NJ)                                                                                                            \
    if (nj == NJ) {                                                                                                           \
        if (vec)                                                                                                              \
            hipLaunchKernelGGL((srx_dense_quant_kernel<NJ, true, MODE>), dim3(blocks), dim3(THREADS), 0, stream, a);          \
        else                                                                                                                  \
            hipLaunchKernelGGL((srx_dense_quant_kernel<NJ, false, MODE>), dim3(blocks), dim3(THREADS), 0, stream, a);         \
        return;                                                                                                               \
    }
    SRX_DQ(1) SRX_DQ(2) SRX_DQ(3) SRX_DQ(4)
#undef SRX_DQ
}

// The checks the four forms share, then the launch.  A query call is a corpus of nq rows quantised from row 0.
int dense_quantize(const char *who, int mode, int32_t device, const float *in, int64_t ld, int64_t n_rows, int32_t dim, int32_t dim_pad,
                   int64_t row0, int64_t n_total, int32_t packed, void *out_codes, float *out_scale, float *out_deq, int32_t *flag,
                   void *stream_v) {
    const bool is_u8 = mode == DQ_U8_ROW || mode == DQ_U8_QUERY;
    if (n_rows < 0 || row0 < 0 || n_total < 0) return fail(SRX_ERR_INVALID, "%s: negative count", who);
    if (row0 > n_total || n_rows > n_total - row0) return fail(SRX_ERR_INVALID, "%s: row0 + n_rows > n_total", who);
    if (dim < 1 || dim > dim_pad || dim_pad > 1024 || ld < dim) return fail(SRX_ERR_INVALID, "%s: need 1 <= dim <= dim_pad <= 1024 and ld >= dim", who);
    if (is_u8) {
        if (dim_pad % 64 != 0) return fail(SRX_ERR_INVALID, "%s: unsupported dim_pad (a multiple of 64)", who);
    } else {
        static const int dims[] = {32, 64, 96, 128, 192, 256, 384, 512, 768, 1024};  // the INT8 engine's row lengths
        bool ok = false;
        for (int d : dims) ok = ok || d == dim_pad;
        if (!ok) return fail(SRX_ERR_INVALID, "%s: unsupported dim_pad (32, 64, 96, 128, 192, 256, 384, 512, 768 or 1024)", who);
    }
    if (packed != 0 && packed != 1) return fail(SRX_ERR_INVALID, "%s: packed must be 0 or 1", who);
    if (packed && (row0 & 31) != 0) return fail(SRX_ERR_INVALID, "%s: row0 must be a multiple of 32 with packed", who);
    if ((n_rows + DQ_TILE - 1) / DQ_TILE > 0x7FFFFFFFll) return fail(SRX_ERR_INVALID, "%s: too many rows in one call", who);
    if (n_rows == 0) return SRX_OK;
    const bool optional = mode == DQ_U8_QUERY;  // codes and scales of the u8 query call
    if (!in || (!optional && (!out_codes || !out_scale)) || (mode == DQ_U8_QUERY && !out_deq)) return fail(SRX_ERR_INVALID, "%s: null pointer", who);
    if ((uintptr_t)in & 3) return fail(SRX_ERR_INVALID, "%s: input must be 4-byte aligned", who);
    if (((uintptr_t)out_codes | (uintptr_t)out_deq) & 15) return fail(SRX_ERR_INVALID, "%s: outputs must be 16-byte aligned", who);
    HIP_TRY(hipSetDevice(device));
    const DenseQuantArgs a = {in, ld, n_rows, row0, n_total, dim, dim_pad, packed, out_codes, out_scale, out_deq, flag};
    const bool vec = ((uintptr_t)in & 15) == 0 && ld % 4 == 0 && dim % 4 == 0;
    const hipStream_t stream = (hipStream_t)stream_v;
    switch (mode) {
        case DQ_I8_ROW: dq_launch<DQ_I8_ROW>(a, vec, stream); break;
        case DQ_I8_QUERY: dq_launch<DQ_I8_QUERY>(a, vec, stream); break;
        case DQ_U8_ROW: dq_launch<DQ_U8_ROW>(a, vec, stream); break;
        default: dq_launch<DQ_U8_QUERY>(a, vec, stream); break;
    }
    HIP_TRY(hipGetLastError());
    return SRX_OK;
}

}  // namespace

SRX_API int srx_dense_quantize_i8(int32_t device, const float *emb, int64_t ld, int64_t n_rows, int32_t dim, int32_t dim_pad, int64_t row0,
                                  int64_t n_total, int32_t packed, void *out_corpus, float *out_scale, int32_t *flag, void *stream) {
    return dense_quantize("srx_dense_quantize_i8", DQ_I8_ROW, device, emb, ld, n_rows, dim, dim_pad, row0, n_total, packed, out_corpus, out_scale,
                          nullptr, flag, stream);
}

SRX_API int srx_dense_quantize_u8(int32_t device, const float *emb, int64_t ld, int64_t n_rows, int32_t dim, int32_t dim_pad, int64_t row0,
                                  int64_t n_total, uint8_t *out_corpus, float *out_scales, int32_t *flag, void *stream) {
    return dense_quantize("srx_dense_quantize_u8", DQ_U8_ROW, device, emb, ld, n_rows, dim, dim_pad, row0, n_total, 0, out_corpus, out_scales,
                          nullptr, flag, stream);
}

SRX_API int srx_dense_quantize_queries_i8(int32_t device, const float *q, int64_t ld, int32_t nq, int32_t dim, int32_t dim_pad, int8_t *out_q,
                                          float *out_scale, int32_t *flag, void *stream) {
    return dense_quantize("srx_dense_quantize_queries_i8", DQ_I8_QUERY, device, q, ld, nq, dim, dim_pad, 0, nq, 0, out_q, out_scale, nullptr, flag,
                          stream);
}

SRX_API int srx_dense_quantize_queries_u8(int32_t device, const float *q, int64_t ld, int32_t nq, int32_t dim, int32_t dim_pad, uint8_t *out_q,
                                          float *out_scales, float *out_deq, int32_t *flag, void *stream) {
    return dense_quantize("srx_dense_quantize_queries_u8", DQ_U8_QUERY, device, q, ld, nq, dim, dim_pad, 0, nq, 0, out_q, out_scales, out_deq, flag,
                          stream);
}
