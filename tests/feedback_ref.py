"""Restatement of include/ext/sparse_rx_feedback.h in plain NumPy / Python, written from the header's contract and not from the
kernel: the row order of the forward index and the expansion of one batch.  Every operation is one float32 operation (NumPy
scalars: no fused multiply-add, IEEE divide); every sum runs in the order the contract names.  The tests compare the engine
against this file, never against itself."""
import numpy as np

BY_SCORE, UNIFORM = 0, 1
RM, RAW = 0, 1
MAX_DOCS, MAX_ENTRIES, MAX_TERMS, MAX_QTERMS = 32, 4096, 128, 128
F32 = np.float32


def forward_rows(indptr, indices, data, idf):
    """The forward index of a CSR: (row_ptr i64, term i32, value f32, max_row_terms).  Inside a row the order is
    key = f32(value * idf[term]) descending, then term ascending; keys compare as floats, so -0 equals +0."""
    indptr = np.asarray(indptr, dtype=np.int64)
    term = np.asarray(indices, dtype=np.int32)
    value = np.asarray(data, dtype=np.float32)
    idf = np.asarray(idf, dtype=np.float32)
    out_t, out_v = np.empty_like(term), np.empty_like(value)
    longest = 0
    for d in range(len(indptr) - 1):
        lo, hi = int(indptr[d]), int(indptr[d + 1])
        longest = max(longest, hi - lo)
        entries = [(F32(value[j] * idf[term[j]]), int(term[j]), j) for j in range(lo, hi)]
        # Python's sort is stable: by term first, then by key descending with float comparison (-0.0 == 0.0)
        entries.sort(key=lambda e: e[1])
        entries.sort(key=lambda e: -float(e[0]))
        for at, (_, _, j) in enumerate(entries):
            out_t[lo + at], out_v[lo + at] = term[j], value[j]
    return indptr.copy(), out_t, out_v, longest


def expand(row_ptr, term, value, doc_len, n_docs, doc_base, fb_docs, row_cap, n_terms, doc_weight, term_weight, alpha, beta, term_gain,
           q_ptr, q_term, q_weight, fb_doc, fb_score, fb_count):
    """-> (out_ptr i32[nq + 1], out_term i32, out_weight f32, flag).  fb_doc / fb_score: [nq, m]; fb_count: [nq] or None;
    term_gain: f32[vocab] or None; doc_len: f32[n_docs] or None (RAW)."""
    alpha, beta = F32(alpha), F32(beta)
    fb_doc = np.asarray(fb_doc)
    nq, m = len(q_ptr) - 1, fb_doc.shape[1]
    out_ptr, out_term, out_weight, flag = [0], [], [], 0
    for q in range(nq):
        qt = [int(t) for t in q_term[q_ptr[q]: q_ptr[q + 1]]]
        qw = [F32(w) for w in q_weight[q_ptr[q]: q_ptr[q + 1]]]
        if len(qt) > MAX_QTERMS:  # copied through unchanged
            flag |= 1
            out_term += qt
            out_weight += qw
            out_ptr.append(len(out_term))
            continue
        limit = min(max(int(fb_count[q]), 0), m, fb_docs) if fb_count is not None else min(m, fb_docs)
        used = []
        for r in range(limit):
            local = int(fb_doc[q, r]) - int(doc_base)
            if not 0 <= local < n_docs:
                continue
            if doc_weight == BY_SCORE and not (F32(0) < F32(fb_score[q, r]) < F32(np.inf)):
                continue
            used.append((r, local))
        if doc_weight == BY_SCORE:
            S = F32(0)
            for r, _ in used:
                S = F32(S + F32(fb_score[q, r]))
        fb = {}
        with np.errstate(all="ignore"):
            for r, d in used:
                a_r = F32(F32(fb_score[q, r]) / S) if doc_weight == BY_SCORE else F32(F32(1) / F32(len(used)))
                lo, hi = int(row_ptr[d]), int(row_ptr[d + 1])
                for j in range(lo, lo + min(hi - lo, row_cap)):
                    p = F32(F32(value[j]) / F32(doc_len[d])) if term_weight == RM else F32(value[j])
                    c = F32(a_r * p)
                    t = int(term[j])
                    fb[t] = F32(fb.get(t, F32(0)) + c)
            gain = (lambda t: F32(1)) if term_gain is None else (lambda t: F32(term_gain[t]))
            cands = [(t, f) for t, f in fb.items() if gain(t) > 0 and f > 0]
            cands.sort(key=lambda e: (-float(F32(e[1] * gain(e[0]))), e[0]))
            selected = dict(cands[:n_terms])
            Fsum = F32(0)
            for t in sorted(selected):
                Fsum = F32(Fsum + selected[t])
            Q = F32(0)
            for w in qw:
                Q = F32(Q + w)
            in_query = dict(zip(qt, qw))
            for t in sorted(set(qt) | set(selected)):
                A = F32(alpha * F32(in_query[t] / Q)) if t in in_query and Q > 0 else F32(0)
                B = F32(beta * F32(selected[t] / Fsum)) if t in selected else F32(0)
                w = F32(A + B)
                if w > 0:
                    out_term.append(t)
                    out_weight.append(w)
        out_ptr.append(len(out_term))
    return (np.asarray(out_ptr, dtype=np.int32), np.asarray(out_term, dtype=np.int32), np.asarray(out_weight, dtype=np.float32), flag)
