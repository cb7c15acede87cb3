"""The chained filter spec on the GPU: ``SparseBackend.filter_spec(...).on_device(index)`` -- doc rows, then term rows over them,
then field rows over those -- against the NumPy AND of the three masks (the doc list, tests/terms_ref.py, tests/fields_ref.py),
word for word.  The corpus is chosen for the builders' edges: 4 133 docs in units of 3 tiles of 64 = 192 docs (a chunk of the
terms kernel is 6 words: its 4-byte store path), three chunks of the fields kernel with the last one partial, and 130 doc words
in rows of 132 (two padding words)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import fields_ref  # noqa: E402
import terms_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N_DOCS, TILE_LOG2, UNIT_TILES = 4_133, 6, 3
DEVICE = "cuda:0"


def test_chained_spec_rows_are_the_and_of_the_three_masks():
    import torch
    assert torch.cuda.is_available(), "this test needs the MI355X"
    import sparse_rx
    from sparse_rx.backend import SparseBackend
    from sparse_rx.filter import filter_words, pack_masks
    from sparse_rx.index import build_host_index

    rng = np.random.default_rng(77)
    words = [f"w{t}" for t in range(40)]
    ids = [f"d{i}" for i in range(N_DOCS)]
    corpus = {d: {"text": " ".join(rng.choice(words, size=6))} for d in ids}
    year = rng.integers(1990, 2024, N_DOCS).astype(np.int32)
    src = [("wiki", "web", "arxiv", None)[i] for i in rng.integers(0, 4, N_DOCS)]
    host = build_host_index(corpus)
    terms_ref.assert_no_stored_zero(host.data)
    be = SparseBackend(DEVICE, TILE_LOG2)
    be.set_host(host)
    be.dev = sparse_rx.DeviceIndex.from_host_index(host, device=DEVICE, tile_log2=TILE_LOG2, unit_tiles=UNIT_TILES)
    assert be.dev.unit_tiles == UNIT_TILES and (UNIT_TILES << TILE_LOG2) == 192 and filter_words(N_DOCS) == 132
    be.set_fields({"year": year, "src": src})

    queries = {"a": "w1 w2", "b": "w3", "c": "w4 w5", "d": "w6"}
    out_a, out_c = ids[5:4_000:7] + [ids[-1]], ids[100:4_133:3]
    excluded_docs = {"a": out_a, "c": out_c}
    must_terms, any_terms, must_not_terms = {"a": ["w3"], "b": ["w7"]}, {"b": ["w1", "w30", "nosuchword"]}, {"a": ["w9"], "b": ["w10"]}
    recent, not_web = {"field": "year", "gte": 2005}, {"field": "src", "eq": "web"}
    where = {"a": {"must": [recent], "must_not": [not_web]}, "c": {"should": [{"field": "src", "in": ["wiki", "arxiv"]}, {"field": "year", "lt": 1995}]}}
    spec = be.filter_spec(queries, excluded_docs=excluded_docs, must_terms=must_terms, any_terms=any_terms, must_not_terms=must_not_terms,
                          where=where, call="search")
    assert spec.row_of_qid["d"] == -1 and sorted(spec.row_of_qid[q] for q in "abc") == [0, 1, 2]

    # the three masks of every qid, each from its own restatement
    def doc_mask(out):
        m = np.ones(N_DOCS, bool)
        m[[int(d[1:]) for d in out]] = False
        return m

    def term_mask(qid):
        tid = lambda ws: [int(host.vocabulary.get(w, -1)) for w in ws]
        lists = [[tid(kw.get(qid, []))] for kw in (must_terms, any_terms, must_not_terms)]
        return terms_ref.term_masks(host.indptr, host.indices, N_DOCS, *lists)[0]

    w = lambda values, clause: np.asarray(fields_ref.where_mask(values, clause), bool)
    every = np.ones(N_DOCS, bool)
    expect = {"a": doc_mask(out_a) & term_mask("a") & w(year, recent) & ~w(src, not_web),
              "b": every & term_mask("b"),
              "c": doc_mask(out_c) & (w(src, where["c"]["should"][0]) | w(year, where["c"]["should"][1]))}
    assert all(50 < m.sum() < N_DOCS - 50 for m in expect.values()), {q: int(m.sum()) for q, m in expect.items()}
    assert not expect["a"][N_DOCS - 1] and expect["c"][4_096:].any()  # the partial last chunk holds set and cleared bits

    dense = sparse_rx.DenseF32Index(rng.standard_normal((N_DOCS, 8)).astype(np.float32), device=DEVICE)
    try:
        for index in (be.dev, dense):
            f = spec.on_device(index)
            assert (f.n_filters, f.n_docs, f.doc_base, f.words) == (3, N_DOCS, 0, 132) and f.for_index(index) is f
            bits = f.bits.cpu().numpy().view(np.uint32)
            for qid, mask in expect.items():
                got, exp = bits[spec.row_of_qid[qid]], pack_masks(mask)[0]
                assert exp.shape == (132,) and not exp[130:].any()
                bad = np.flatnonzero(got != exp)
                assert bad.size == 0, f"{type(index).__name__} qid {qid}: {bad.size} words differ, first {bad[:4].tolist()}"
    finally:
        be.close()
