"""NumPy restatement of include/sparse_rx_terms.h, written from the header: which docs a (must all / must any / must none)
triple of term lists allows.  Computed from the doc-major CSR an index was built from, never from the engine.  Packing the
masks into filter rows is filter_ref.pack / sparse_rx.filter.pack_masks.  Shared by test_terms_cpu.py and test_terms_gpu.py."""
import numpy as np


def assert_no_stored_zero(data):
    """The header's rule is about STORED postings (an explicit zero is one); the restatement below reads the CSR's entries, so
    the two agree on any corpus -- but the oracle rankings the GPU tests compare with only know non-zero contributions.  The
    fixture corpora hold no explicitly stored zero, so "stored posting" and "non-zero entry" coincide on them."""
    assert np.all(np.asarray(data) != 0), "a fixture corpus holds an explicitly stored zero"


def docs_with_term(indptr, indices, n_docs, t):
    """bool[n_docs]: doc d has an entry of term t (duplicates are one posting; -1 is the term no doc has)"""
    has = np.zeros(n_docs, dtype=bool)
    if t < 0:
        return has
    indptr = np.asarray(indptr, dtype=np.int64)
    rows = np.repeat(np.arange(n_docs), np.diff(indptr))
    has[rows[np.asarray(indices) == t]] = True
    return has


def term_masks(indptr, indices, n_docs, all=None, any=None, none=None, base_masks=None, q_base=None):
    """bool[n_rows, n_docs].  all / any / none: None (no such list) or one list of term ids per row; base_masks None or
    bool[n_base, n_docs]; q_base None (base row 0 for every row) or one base row per OUTPUT row, -1 = every doc."""
    n_rows = max(len(x) for x in (all, any, none) if x is not None)
    cache = {}

    def has(t):
        if t not in cache:
            cache[t] = docs_with_term(indptr, indices, n_docs, int(t))
        return cache[t]

    out = np.ones((n_rows, n_docs), dtype=bool)
    for r in range(n_rows):
        if base_masks is not None:
            b = 0 if q_base is None else int(q_base[r])
            if b >= 0:
                out[r] &= np.asarray(base_masks, dtype=bool).reshape(-1, n_docs)[b]
        for t in (all[r] if all is not None else ()):
            out[r] &= has(t)
        if any is not None and len(any[r]) > 0:
            one = np.zeros(n_docs, dtype=bool)
            for t in any[r]:
                one |= has(t)
            out[r] &= one
        for t in (none[r] if none is not None else ()):
            out[r] &= ~has(t)
    return out
