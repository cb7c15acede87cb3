// The argument checks that the filter builders and srx_score_docs share, and those of srx_collapse_topk, run on the host under AddressSanitizer and UBSan: every
// refusal below returns before anything touches a device, so the program needs no GPU.  Build and run from the repository root
// (PKG = the package directory):
//
//   for u in filter terms fields score_docs collapse; do
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -fPIC -Xarch_host -fsanitize=address,undefined \
//           -Iinclude -I$PKG/csrc -c $PKG/csrc/$u.hip -o /tmp/fc_$u.o; done
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -Iinclude -c tools/filter_checks_host.cpp -o /tmp/fc_main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/fc_main.o /tmp/fc_filter.o /tmp/fc_terms.o /tmp/fc_fields.o \
//         /tmp/fc_score_docs.o /tmp/fc_collapse.o -o /tmp/filter_checks_host && /tmp/filter_checks_host
//
// (clang++ is the one hipcc drives, <rocm>/llvm/bin/clang++: the two sanitizer runtimes must be the same.)
//
// It prints one line per refusal and "all N refusals as expected"; exit status 1 when a return code or a message differs.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "sparse_rx.h"
#include "sparse_rx_collapse.h"
#include "sparse_rx_fields.h"
#include "sparse_rx_filter.h"
#include "sparse_rx_terms.h"

thread_local char srx_g_err[512] = "";  // sparse_rx.hip defines it in the library; that unit is not linked here

// hidden-visibility host functions of the units (csrc/desc_check.h, csrc/filter_common.h)
int srx_check_index_desc(const char *who, const srx_index_desc *d);
int srx_check_filter(const char *who, const srx_doc_filter *f);
int srx_check_row_builder(const char *who, const char *ids, int32_t n_rows, const int32_t *all_ptr, const int32_t *all_ids, const int32_t *any_ptr,
                          const int32_t *any_ids, const int32_t *none_ptr, const int32_t *none_ids, const uint32_t *out_bits, const srx_doc_filter *base);

static int n_bad = 0, n_seen = 0;

static void expect(int rc, const char *msg) {
    ++n_seen;
    const bool ok = rc == SRX_ERR_INVALID && strcmp(srx_g_err, msg) == 0;
    printf("%s  %s\n", ok ? "ok " : "BAD", msg);
    if (!ok) {
        printf("     got rc %d, \"%s\"\n", rc, srx_g_err);
        ++n_bad;
    }
    srx_g_err[0] = 0;
}

int main() {
    alignas(16) static int32_t mem[64];  // addresses only: no check dereferences a device pointer
    const int32_t *p = mem;
    uint32_t *out = reinterpret_cast<uint32_t *>(mem), *odd = out + 1;

    srx_index_desc d;
    memset(&d, 0, sizeof(d));
    d.val_type = SRX_VAL_F32, d.n_docs = 1000, d.vocab = 50, d.tile_log2 = 6, d.n_tiles = 16, d.unit_tiles = 4;
    d.term_ptr = reinterpret_cast<const int64_t *>(mem), d.post = p, d.tile_skip = p, d.idf = reinterpret_cast<const float *>(mem);
    srx_doc_filter base = {out, 1, nullptr};

    // the descriptor, as both entry points report it
    for (int terms = 0; terms < 2; ++terms) {
        auto call = [&](const srx_index_desc *dd) {
            return terms ? srx_filter_from_terms(dd, 1, p, p, nullptr, nullptr, nullptr, nullptr, nullptr, out, nullptr)
                         : srx_score_docs(dd, p, p, reinterpret_cast<const float *>(mem), 1, p, nullptr, 1, reinterpret_cast<float *>(mem), nullptr);
        };
        const char *who = terms ? "srx_filter_from_terms" : "srx_score_docs";
        char msg[256];
        auto said = [&](const char *what) { snprintf(msg, sizeof(msg), "%s: %s", who, what); return msg; };
        expect(call(nullptr), said("null descriptor"));
        srx_index_desc b = d;
        b.val_type = 7;
        expect(call(&b), said("bad val_type"));
        b = d, b.n_docs = 0;
        expect(call(&b), said("n_docs / vocab out of range"));
        b = d, b.n_docs = 0x7FFFFFFFll;
        expect(call(&b), said("n_docs / vocab out of range"));
        b = d, b.tile_log2 = 5;
        expect(call(&b), said("tile_log2 must be in [6, 14]"));
        b = d, b.tile_log2 = 15;
        expect(call(&b), said("tile_log2 must be in [6, 14]"));
        b = d, b.n_tiles = 15;
        expect(call(&b), said("n_tiles != ceil(n_docs / 2^tile_log2)"));
        b = d, b.unit_tiles = 65;
        expect(call(&b), said("unit_tiles must be in [1, 64]"));
        b = d, b.post = nullptr;
        expect(call(&b), said("the descriptor has neither post nor post16"));
        b = d, b.tile_log2 = 14, b.n_tiles = 1, b.post16 = p;
        expect(call(&b), said("a compact copy (post16) needs units of <= 49152 docs"));
        b = d, b.idf = nullptr;
        expect(call(&b), said("null term_ptr / tile_skip / idf"));
        expect(srx_check_index_desc(who, nullptr), said("null descriptor"));
    }

    // what the two builders share, through each entry point
    srx_field_col col = {mem, nullptr, SRX_FIELD_I32};
    for (int fields = 0; fields < 2; ++fields) {
        auto call = [&](int32_t n_rows, const int32_t *ap, const int32_t *ai, const int32_t *yp, const int32_t *yi, const int32_t *np_, const int32_t *ni,
                        const srx_doc_filter *bs, uint32_t *o) {
            return fields ? srx_filter_from_fields(0, 1000, &col, 1, nullptr, 0, nullptr, n_rows, ap, ai, yp, yi, np_, ni, bs, o, nullptr)
                          : srx_filter_from_terms(&d, n_rows, ap, ai, yp, yi, np_, ni, bs, o, nullptr);
        };
        const char *who = fields ? "srx_filter_from_fields" : "srx_filter_from_terms";
        char msg[256];
        auto said = [&](const char *what) { snprintf(msg, sizeof(msg), "%s: %s", who, what); return msg; };
        const char *together = fields ? "the ptr and clause arrays of a list go together (both or neither)"
                                      : "the ptr and term arrays of a list go together (both or neither)";
        expect(call(-1, p, p, nullptr, nullptr, nullptr, nullptr, nullptr, out), said("n_rows < 0"));
        expect(call(1, p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, out), said(together));
        expect(call(1, p, p, nullptr, p, nullptr, nullptr, nullptr, out), said(together));
        expect(call(1, p, p, nullptr, nullptr, p, nullptr, nullptr, out), said(together));
        expect(call(1, p, p, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), said("null out_bits"));
        expect(call(1, p, p, nullptr, nullptr, nullptr, nullptr, nullptr, odd), said("filter rows must be 16-byte aligned"));
        srx_doc_filter b = base;
        b.bits = nullptr;
        expect(call(1, p, p, nullptr, nullptr, nullptr, nullptr, &b, out), said("null filter bits"));
        b = base, b.bits = odd;
        expect(call(1, p, p, nullptr, nullptr, nullptr, nullptr, &b, out), said("filter rows must be 16-byte aligned"));
        b = base, b.n_filters = 0;
        expect(call(1, p, p, nullptr, nullptr, nullptr, nullptr, &b, out), said("n_filters must be >= 1"));
        expect(srx_check_filter(who, nullptr), said("null filter"));
        expect(srx_check_row_builder(who, fields ? "clause" : "term", 1, nullptr, p, nullptr, nullptr, nullptr, nullptr, out, nullptr), said(together));
        // n_rows = 0 with everything else in order: nothing to do, no device touched
        ++n_seen;
        if (call(0, p, p, nullptr, nullptr, nullptr, nullptr, &base, out) != SRX_OK) ++n_bad, printf("BAD  %s: n_rows = 0 refused\n", who);
    }
    // srx_collapse_topk: its checks are its own
    {
        float *fs = reinterpret_cast<float *>(mem);
        int32_t *o = mem;
        auto call = [&](const srx_field_col *c, int64_t n_docs, int64_t doc_base, const int32_t *cd, const float *cs, int32_t nq, int32_t m, int32_t k,
                        int32_t per_group, int32_t policy, int32_t *od, float *os, int32_t *oc) {
            return srx_collapse_topk(0, c, n_docs, doc_base, cd, cs, nullptr, nq, m, k, per_group, policy, od, os, oc, nullptr, nullptr, nullptr);
        };
        const char *who = "srx_collapse_topk";
        char msg[256];
        auto said = [&](const char *what) { snprintf(msg, sizeof(msg), "%s: %s", who, what); return msg; };
        srx_field_col c64 = {mem, reinterpret_cast<const uint32_t *>(mem), SRX_FIELD_I64}, b = c64;
        expect(call(nullptr, 1000, 0, p, fs, 1, 8, 4, 1, 0, o, fs, o), said("null col"));
        b.type = SRX_FIELD_F32;
        expect(call(&b, 1000, 0, p, fs, 1, 8, 4, 1, 0, o, fs, o), said("the column must be SRX_FIELD_I32 or SRX_FIELD_I64 (F32 and SET64 columns are no group keys)"));
        b.type = SRX_FIELD_SET64;
        expect(call(&b, 1000, 0, p, fs, 1, 8, 4, 1, 0, o, fs, o), said("the column must be SRX_FIELD_I32 or SRX_FIELD_I64 (F32 and SET64 columns are no group keys)"));
        b = c64, b.data = nullptr;
        expect(call(&b, 1000, 0, p, fs, 1, 8, 4, 1, 0, o, fs, o), said("a column with null data"));
        b = c64, b.data = mem + 1;
        expect(call(&b, 1000, 0, p, fs, 1, 8, 4, 1, 0, o, fs, o), said("column data must be aligned for its type"));
        b = c64, b.valid = odd;
        expect(call(&b, 1000, 0, p, fs, 1, 8, 4, 1, 0, o, fs, o), said("a validity row must be 16-byte aligned"));
        expect(call(&c64, 0, 0, p, fs, 1, 8, 4, 1, 0, o, fs, o), said("n_docs must be in [1, 2^31 - 2]"));
        expect(call(&c64, 0x7FFFFFFFll, 0, p, fs, 1, 8, 4, 1, 0, o, fs, o), said("n_docs must be in [1, 2^31 - 2]"));
        expect(call(&c64, 1000, -1, p, fs, 1, 8, 4, 1, 0, o, fs, o), said("negative doc_base"));
        expect(call(&c64, 1000, 0, p, fs, 1, 0, 1, 1, 0, o, fs, o), said("m must be in [1, 2048]"));
        expect(call(&c64, 1000, 0, p, fs, 1, 2049, 1, 1, 0, o, fs, o), said("m must be in [1, 2048]"));
        expect(call(&c64, 1000, 0, p, fs, 1, 8, 0, 1, 0, o, fs, o), said("k must be in [1, m]"));
        expect(call(&c64, 1000, 0, p, fs, 1, 8, 9, 1, 0, o, fs, o), said("k must be in [1, m]"));
        expect(call(&c64, 1000, 0, p, fs, 1, 8, 4, 0, 0, o, fs, o), said("per_group must be >= 1"));
        expect(call(&c64, 1000, 0, p, fs, 1, 8, 4, 1, 3, o, fs, o), said("unknown null_policy"));
        expect(call(&c64, 1000, 0, p, fs, 1, 8, 4, 1, -1, o, fs, o), said("unknown null_policy"));
        expect(call(&c64, 1000, 0, p, fs, -1, 8, 4, 1, 0, o, fs, o), said("nq < 0"));
        expect(call(&c64, 1000, 0, p, fs, 1 << 20, 2048, 4, 1, 0, o, fs, o), said("nq * m must not exceed 2^31 - 1"));
        expect(call(&c64, 1000, 0, nullptr, fs, 1, 8, 4, 1, 0, o, fs, o), said("null cand_doc / cand_score"));
        expect(call(&c64, 1000, 0, p, nullptr, 1, 8, 4, 1, 0, o, fs, o), said("null cand_doc / cand_score"));
        expect(call(&c64, 1000, 0, p, fs, 1, 8, 4, 1, 0, nullptr, fs, o), said("null out_doc / out_score / out_count"));
        expect(call(&c64, 1000, 0, p, fs, 1, 8, 4, 1, 0, o, nullptr, o), said("null out_doc / out_score / out_count"));
        expect(call(&c64, 1000, 0, p, fs, 1, 8, 4, 1, 0, o, fs, nullptr), said("null out_doc / out_score / out_count"));
        // nq = 0 with everything else in order: nothing to do, no device touched
        ++n_seen;
        if (call(&c64, 1000, 0, nullptr, nullptr, 0, 2048, 2048, 0x7FFFFFFF, 2, nullptr, nullptr, nullptr) != SRX_OK) ++n_bad, printf("BAD  %s: nq = 0 refused\n", who);
    }
    if (n_bad) {
        printf("%d of %d checks differ\n", n_bad, n_seen);
        return 1;
    }
    printf("all %d refusals as expected\n", n_seen);
    return 0;
}
