"""The rows include/late/sparse_rx_maxsim_search.h promises, from a GIVEN score matrix: query q's row is the rerank rule of
tests/late_ref.py (score descending, doc ascending, -1 / +0 padding) over ALL docs its mask allows.  Never calls the engine."""
import numpy as np

import late_ref


def expected(scores, allowed, k, doc_base=0):
    """scores f32[nq, n_docs], allowed bool[nq, n_docs] (None: every doc) -> (doc i32[nq, k], score f32[nq, k], count i32[nq])"""
    scores = np.asarray(scores, dtype=np.float32)
    nq, n_docs = scores.shape
    docs = doc_base + np.arange(n_docs, dtype=np.int64)
    out = np.full((nq, k), -1, np.int32), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)
    for q in range(nq):
        live = np.ones(n_docs, bool) if allowed is None else np.asarray(allowed[q], dtype=bool)
        out[0][q], out[1][q], out[2][q] = late_ref.rank(docs, scores[q], live, k)
    return out
