"""The ORDER of the refusals of the seven entry points over metadata columns (srx_filter_from_fields, srx_collapse_topk,
srx_facet_counts, srx_facet_counts_lists, srx_order_topk, srx_order_lists, srx_boost_topk) and of the FieldTable doors in
front of them: a call with two faults names the one its checks meet first, ``nq == 0`` / ``n_rows == 0`` is fine whatever the
pointers are but only after the checks in front of it, and which entry points bound ``doc_base + n_docs``.  No GPU: the
addresses are never dereferenced and the doors refuse before any device call."""
import ctypes

import numpy as np
import pytest
import torch

from sparse_rx import _capi, fields
from sparse_rx.filter import DocFilter

P = [(i + 1) << 20 for i in range(24)]  # 16-byte aligned addresses, never dereferenced
I32_MAX = 2 ** 31 - 1
I32, I64, F32, SET64 = 0, 1, 2, 3


def _cols(*specs):
    arr = (_capi.FieldColDesc * len(specs))()
    for i, (data, valid, typ) in enumerate(specs):
        arr[i].data, arr[i].valid, arr[i].type = data, valid, typ
    return arr


def _bins(mode=0, n_bins=8, origin=0, edges=None):
    return ctypes.pointer(_capi.FacetBins(mode=mode, n_bins=n_bins, origin=origin, edges=edges))


def _flt(bits=P[2], n_filters=2, q_filter=P[4]):
    return ctypes.pointer(_capi.DocFilterDesc(bits=bits, n_filters=n_filters, q_filter=q_filter))


GOOD = (P[0], P[1], I64)           # a column every entry point takes
ODD = (P[0] + 2, P[1], I64)        # its data misaligned
NO_DATA = (None, None, I64)
BAD_VALID = (P[0], P[1] + 4, I64)

# the arguments of a good call, in the order of the C signature
OK = {
    "srx_filter_from_fields": dict(device=0, n_docs=1000, cols=_cols(GOOD, (P[2], None, F32)), n_cols=2, clauses=P[5], n_clauses=3, values=None, n_rows=3,
                                   all_ptr=P[6], all_clause=P[7], any_ptr=None, any_clause=None, none_ptr=P[9], none_clause=P[10], base=None,
                                   out=P[11], stream=None),
    "srx_collapse_topk": dict(device=0, col=_cols(GOOD), n_docs=1000, doc_base=0, cand_doc=P[2], cand_score=P[3], cand_count=P[4], nq=3, m=100, k=10,
                              per_group=1, null_policy=0, out_doc=P[5], out_score=P[6], out_count=P[7], out_pos=P[8], out_group=P[9], stream=None),
    "srx_facet_counts": dict(device=0, col=_cols(GOOD), n_docs=1000, bins=_bins(), filter=_flt(), n_rows=3, out_counts=P[5], out_extra=P[6],
                             stream=None),
    "srx_facet_counts_lists": dict(device=0, col=_cols(GOOD), n_docs=1000, doc_base=0, bins=_bins(), cand_doc=P[2], cand_count=P[3], nq=3, m=100,
                                   out_counts=P[5], out_extra=P[6], stream=None),
    "srx_order_topk": dict(device=0, col=_cols(GOOD), n_docs=1000, doc_base=0, order=1, nulls=0, filter=_flt(), n_rows=3, k=10, after_doc=P[5],
                           out_doc=P[6], out_key=P[7], out_extra=P[8], workspace=P[9], workspace_bytes=3 * 128, stream=None),
    "srx_order_lists": dict(device=0, col=_cols(GOOD), n_docs=1000, doc_base=0, order=0, nulls=1, cand_doc=P[2], cand_score=P[3], cand_count=P[4],
                            nq=3, m=100, k=10, out_doc=P[5], out_score=P[6], out_key=P[7], out_pos=P[8], out_extra=P[9], stream=None),
    "srx_boost_topk": dict(device=0, cols=_cols(GOOD, (P[2], None, F32)), n_cols=2, n_docs=1000, doc_base=0, clauses=P[4], n_clauses=2, knots=P[5],
                           n_knots=300, score_mode=0, boost_mode=0, cand_doc=P[6], cand_score=P[7], cand_count=P[8], carry_doc=P[9],
                           carry_score=P[10], carry_count=P[11], nq=3, m=100, kc=10, k=10, out_doc=P[12], out_score=P[13], out_count=P[14],
                           out_pos=P[15], stream=None),
}
COL = {name: "cols" if name in ("srx_filter_from_fields", "srx_boost_topk") else "col" for name in OK}


def _with_col(name, spec):
    """the call's column argument with its first column replaced"""
    second = [(P[2], None, F32)] if COL[name] == "cols" else []
    return {COL[name]: _cols(spec, *second)}


N_DOCS, ALIGNED, NULL_DATA, VALID16, UNKNOWN = ("n_docs must be in [1, 2^31 - 2]", "column data must be aligned for its type", "a column with null data",
                                                "a validity row must be 16-byte aligned", "unknown column type")
NO_OUT = dict(out_doc=None, out_score=None, out_count=None, out_pos=None)
NO_CAND = dict(cand_doc=None, cand_score=None, cand_count=None)

# (entry point, what differs from the good call, the message that wins -- None: the call returns SRX_OK)
CASES = [
    # ---- srx_filter_from_fields: n_docs, n_cols, the columns, the clauses, the row builder's checks, n_rows == 0
    ("srx_filter_from_fields", dict(_with_col("srx_filter_from_fields", ODD), n_docs=0), N_DOCS),
    ("srx_filter_from_fields", dict(n_docs=0, n_cols=33), N_DOCS),
    ("srx_filter_from_fields", dict(_with_col("srx_filter_from_fields", ODD), n_cols=0), "n_cols must be in [1, 32]"),
    ("srx_filter_from_fields", dict(_with_col("srx_filter_from_fields", (None, None, 7))), UNKNOWN),
    ("srx_filter_from_fields", dict(_with_col("srx_filter_from_fields", (None, P[1] + 4, SET64))), NULL_DATA),
    ("srx_filter_from_fields", dict(_with_col("srx_filter_from_fields", (P[0] + 4, P[1] + 4, SET64))), ALIGNED),
    ("srx_filter_from_fields", dict(_with_col("srx_filter_from_fields", BAD_VALID), n_clauses=-1), VALID16),
    ("srx_filter_from_fields", dict(cols=_cols(GOOD, (P[2] + 2, None, F32)), n_clauses=-1), ALIGNED),  # the second column is checked too
    ("srx_filter_from_fields", dict(n_clauses=-1, n_rows=-1), "n_clauses < 0"),
    ("srx_filter_from_fields", dict(n_rows=0, clauses=None, n_clauses=0, all_ptr=None, all_clause=None, none_ptr=None, none_clause=None), None),
    ("srx_filter_from_fields", dict(n_rows=0, clauses=None), "null clauses"),
    ("srx_filter_from_fields", dict(n_rows=0, out=None), "null out_bits"),
    ("srx_filter_from_fields", dict(n_rows=0, n_clauses=-1), "n_clauses < 0"),
    ("srx_filter_from_fields", dict(_with_col("srx_filter_from_fields", ODD), n_rows=0), ALIGNED),
    # ---- srx_collapse_topk: the column, n_docs, doc_base, m, k, per_group, null_policy, nq, nq * m, nq == 0, the pointers
    ("srx_collapse_topk", dict(_with_col("srx_collapse_topk", ODD), n_docs=0), ALIGNED),
    ("srx_collapse_topk", dict(_with_col("srx_collapse_topk", (None, None, F32))), "SRX_FIELD_I32 or SRX_FIELD_I64"),
    ("srx_collapse_topk", dict(_with_col("srx_collapse_topk", (None, None, 7))), "SRX_FIELD_I32 or SRX_FIELD_I64"),
    ("srx_collapse_topk", dict(_with_col("srx_collapse_topk", (None, P[1] + 4, I32))), NULL_DATA),
    ("srx_collapse_topk", dict(_with_col("srx_collapse_topk", BAD_VALID), n_docs=0), VALID16),
    ("srx_collapse_topk", dict(n_docs=0, m=0), N_DOCS),
    ("srx_collapse_topk", dict(n_docs=0, doc_base=-1), N_DOCS),
    ("srx_collapse_topk", dict(doc_base=-1, m=0), "negative doc_base"),
    ("srx_collapse_topk", dict(m=2049, k=0), "m must be in [1, 2048]"),
    ("srx_collapse_topk", dict(k=0, nq=-1), "k must be in [1, m]"),
    ("srx_collapse_topk", dict(k=0, per_group=0), "k must be in [1, m]"),
    ("srx_collapse_topk", dict(per_group=0, null_policy=9), "per_group must be >= 1"),
    ("srx_collapse_topk", dict(null_policy=9, nq=-1), "unknown null_policy"),
    ("srx_collapse_topk", dict(nq=-1, cand_doc=None), "nq < 0"),
    ("srx_collapse_topk", dict(nq=I32_MAX, m=2048, k=1, cand_doc=None), "nq * m must not exceed 2^31 - 1"),
    ("srx_collapse_topk", dict(cand_doc=None, out_doc=None), "null cand_doc / cand_score"),
    ("srx_collapse_topk", dict(out_count=None), "null out_doc / out_score / out_count"),
    ("srx_collapse_topk", dict(nq=0, out_group=None, **NO_CAND, **NO_OUT), None),
    ("srx_collapse_topk", dict(nq=0, k=0), "k must be in [1, m]"),
    ("srx_collapse_topk", dict(nq=0, per_group=0), "per_group must be >= 1"),
    ("srx_collapse_topk", dict(nq=0, doc_base=I32_MAX - 1000), None),           # doc_base + n_docs = 2^31 - 1: no bound here
    ("srx_collapse_topk", dict(nq=0, doc_base=2 ** 40), None),
    # ---- srx_facet_counts: the column, n_docs, the bins, n_rows, the filter, n_rows == 0, the outputs
    ("srx_facet_counts", dict(_with_col("srx_facet_counts", ODD), n_docs=0), ALIGNED),
    ("srx_facet_counts", dict(_with_col("srx_facet_counts", (None, None, 7))), UNKNOWN),
    ("srx_facet_counts", dict(_with_col("srx_facet_counts", (None, P[1] + 4, F32))), NULL_DATA),
    ("srx_facet_counts", dict(n_docs=0, bins=None), N_DOCS),
    ("srx_facet_counts", dict(n_docs=0, n_rows=-1), N_DOCS),
    ("srx_facet_counts", dict(bins=_bins(mode=9), n_rows=-1), "unknown bins mode"),
    ("srx_facet_counts", dict(bins=_bins(mode=1), n_rows=-1), "SRX_FACET_LABELS is for SET64 columns"),
    ("srx_facet_counts", dict(n_rows=-1, filter=_flt(None)), "n_rows < 0"),
    ("srx_facet_counts", dict(filter=_flt(None), out_counts=None), "null filter bits"),
    ("srx_facet_counts", dict(n_rows=0, out_counts=None, out_extra=None), None),
    ("srx_facet_counts", dict(n_rows=0, bins=_bins(n_bins=0)), "n_bins must be in [1, 8192]"),
    ("srx_facet_counts", dict(n_rows=0, filter=_flt(None)), "null filter bits"),
    ("srx_facet_counts", dict(out_extra=None), "null out_counts / out_extra"),
    # ---- srx_facet_counts_lists: the column, n_docs, the bins, doc_base and its bound, nq, m, nq * m, nq == 0, the pointers
    ("srx_facet_counts_lists", dict(_with_col("srx_facet_counts_lists", ODD), n_docs=0), ALIGNED),
    ("srx_facet_counts_lists", dict(_with_col("srx_facet_counts_lists", (None, None, -1))), UNKNOWN),
    ("srx_facet_counts_lists", dict(n_docs=0, m=0), N_DOCS),
    ("srx_facet_counts_lists", dict(n_docs=0, doc_base=-1), N_DOCS),
    ("srx_facet_counts_lists", dict(bins=_bins(n_bins=0), doc_base=-1), "n_bins must be in [1, 8192]"),
    ("srx_facet_counts_lists", dict(doc_base=-1, nq=-1), "negative doc_base"),
    ("srx_facet_counts_lists", dict(doc_base=I32_MAX - 1000, nq=0), "doc_base + n_docs must be below 2^31 - 1"),
    ("srx_facet_counts_lists", dict(doc_base=I32_MAX - 1001, nq=0), None),
    ("srx_facet_counts_lists", dict(doc_base=2 ** 40, nq=-1), "doc_base + n_docs must be below 2^31 - 1"),
    ("srx_facet_counts_lists", dict(nq=-1, m=0), "nq < 0"),
    ("srx_facet_counts_lists", dict(m=0, cand_doc=None), "m must be >= 1"),
    ("srx_facet_counts_lists", dict(nq=I32_MAX, m=3, cand_doc=None), "nq * m must not exceed 2^31 - 1"),
    ("srx_facet_counts_lists", dict(nq=0, cand_doc=None, cand_count=None, out_counts=None, out_extra=None), None),
    ("srx_facet_counts_lists", dict(nq=0, m=0), "m must be >= 1"),
    ("srx_facet_counts_lists", dict(nq=0, m=I32_MAX), None),                     # no cap on m here
    ("srx_facet_counts_lists", dict(cand_doc=None, out_counts=None), "null cand_doc"),
    ("srx_facet_counts_lists", dict(out_extra=None), "null out_counts / out_extra"),
    # ---- srx_order_topk: the column, order, nulls, n_docs, doc_base and its bound, k, n_rows, n_rows * k, the filter, n_rows == 0
    ("srx_order_topk", dict(_with_col("srx_order_topk", ODD), n_docs=0), ALIGNED),
    ("srx_order_topk", dict(_with_col("srx_order_topk", (None, None, SET64))), "a SET64 column has no order"),
    ("srx_order_topk", dict(_with_col("srx_order_topk", (None, None, 7))), UNKNOWN),
    ("srx_order_topk", dict(_with_col("srx_order_topk", (P[0] + 4, None, F32)), order=7), "unknown order"),  # 4 bytes align a float
    ("srx_order_topk", dict(_with_col("srx_order_topk", BAD_VALID), order=7), VALID16),
    ("srx_order_topk", dict(order=7, nulls=7), "unknown order"),
    ("srx_order_topk", dict(nulls=7, n_docs=0), "unknown nulls mode"),
    ("srx_order_topk", dict(n_docs=0, k=0), N_DOCS),
    ("srx_order_topk", dict(n_docs=0, doc_base=-1), N_DOCS),
    ("srx_order_topk", dict(doc_base=-1, k=0), "negative doc_base"),
    ("srx_order_topk", dict(doc_base=I32_MAX - 1000, n_rows=0), "doc_base + n_docs must be below 2^31 - 1"),
    ("srx_order_topk", dict(doc_base=I32_MAX - 1001, n_rows=0), None),
    ("srx_order_topk", dict(k=0, n_rows=-1), "k must be in [1, 1024]"),
    ("srx_order_topk", dict(n_rows=-1, filter=_flt(None)), "n_rows < 0"),
    ("srx_order_topk", dict(n_rows=I32_MAX, k=2, filter=_flt(None)), "n_rows * k must not exceed 2^31 - 1"),
    ("srx_order_topk", dict(filter=_flt(None), out_doc=None), "null filter bits"),
    ("srx_order_topk", dict(n_rows=0, after_doc=None, out_doc=None, out_key=None, out_extra=None, workspace=None, workspace_bytes=0), None),
    ("srx_order_topk", dict(n_rows=0, k=0), "k must be in [1, 1024]"),
    ("srx_order_topk", dict(out_key=None, workspace=None), "null out_doc / out_key / out_extra"),
    # ---- srx_order_lists: the column .. the bound as above, m, k, nq, nq * m, nq == 0, the pointers
    ("srx_order_lists", dict(_with_col("srx_order_lists", ODD), n_docs=0), ALIGNED),
    ("srx_order_lists", dict(_with_col("srx_order_lists", (None, None, SET64))), "a SET64 column has no order"),
    ("srx_order_lists", dict(_with_col("srx_order_lists", (None, None, 4))), UNKNOWN),
    ("srx_order_lists", dict(nulls=7, n_docs=0), "unknown nulls mode"),
    ("srx_order_lists", dict(n_docs=0, m=0), N_DOCS),
    ("srx_order_lists", dict(doc_base=-1, m=0), "negative doc_base"),
    ("srx_order_lists", dict(doc_base=I32_MAX - 1000, m=0), "doc_base + n_docs must be below 2^31 - 1"),
    ("srx_order_lists", dict(doc_base=I32_MAX - 1000, nq=0), "doc_base + n_docs must be below 2^31 - 1"),
    ("srx_order_lists", dict(doc_base=I32_MAX - 1001, nq=0), None),
    ("srx_order_lists", dict(m=2049, k=0), "m must be in [1, 2048]"),
    ("srx_order_lists", dict(k=0, nq=-1), "k must be in [1, m]"),
    ("srx_order_lists", dict(nq=-1, cand_doc=None), "nq < 0"),
    ("srx_order_lists", dict(nq=I32_MAX, m=2048, cand_doc=None), "nq * m must not exceed 2^31 - 1"),
    ("srx_order_lists", dict(nq=0, out_doc=None, out_score=None, out_key=None, out_pos=None, out_extra=None, **NO_CAND), None),
    ("srx_order_lists", dict(nq=0, k=0), "k must be in [1, m]"),
    ("srx_order_lists", dict(cand_score=None, out_doc=None), "null cand_doc / cand_score"),
    ("srx_order_lists", dict(out_extra=None), "null out_doc / out_score / out_key / out_extra"),
    # ---- srx_boost_topk: cols, n_cols, the columns, n_docs, doc_base, the clause counts and modes, m, kc, k, nq, the carry, nq == 0
    ("srx_boost_topk", dict(_with_col("srx_boost_topk", ODD), n_docs=0), ALIGNED),
    ("srx_boost_topk", dict(_with_col("srx_boost_topk", ODD), n_cols=0), "n_cols must be in [1, 8]"),
    ("srx_boost_topk", dict(_with_col("srx_boost_topk", (None, None, SET64))), "a SET64 column is no number to boost by"),
    ("srx_boost_topk", dict(_with_col("srx_boost_topk", (None, None, 7))), UNKNOWN),
    ("srx_boost_topk", dict(_with_col("srx_boost_topk", (None, P[1] + 4, I32))), NULL_DATA),
    ("srx_boost_topk", dict(cols=_cols(BAD_VALID, (P[2], None, SET64))), VALID16),  # column by column: the first one's faults first
    ("srx_boost_topk", dict(cols=_cols(GOOD, (P[2] + 2, None, F32)), n_docs=0), ALIGNED),
    ("srx_boost_topk", dict(n_docs=0, m=0), N_DOCS),
    ("srx_boost_topk", dict(n_docs=0, doc_base=-1), N_DOCS),
    ("srx_boost_topk", dict(doc_base=-1, n_clauses=0), "negative doc_base"),
    ("srx_boost_topk", dict(n_clauses=0, m=0), "n_clauses must be in [1, 8]"),
    ("srx_boost_topk", dict(boost_mode=9, m=0), "unknown boost_mode"),
    ("srx_boost_topk", dict(m=0, kc=-1), "m must be >= 1"),
    ("srx_boost_topk", dict(m=2048, k=0), "m + kc must not exceed 2048"),
    ("srx_boost_topk", dict(k=0, nq=-1), "k must be in [1, m + kc]"),
    ("srx_boost_topk", dict(nq=-1, kc=0), "nq < 0"),
    ("srx_boost_topk", dict(nq=0, kc=0), "a carry given with kc == 0"),
    ("srx_boost_topk", dict(nq=0, clauses=None, knots=None, carry_doc=None, carry_score=None, carry_count=None, **NO_CAND, **NO_OUT), None),
    ("srx_boost_topk", dict(nq=0, k=0), "k must be in [1, m + kc]"),
    ("srx_boost_topk", dict(nq=0, doc_base=I32_MAX - 1000), None),               # doc_base + n_docs = 2^31 - 1: no bound here
    ("srx_boost_topk", dict(nq=0, doc_base=2 ** 40), None),
    ("srx_boost_topk", dict(clauses=None, cand_doc=None), "null clauses / knots"),
    ("srx_boost_topk", dict(cand_doc=None, carry_doc=None), "null cand_doc / cand_score"),
    ("srx_boost_topk", dict(carry_score=None, out_doc=None), "kc > 0 needs carry_doc and carry_score"),
]


@pytest.mark.parametrize("name", list(OK))
def test_first_refusal_of_every_entry_point(name):
    L = _capi.lib()
    fn = getattr(L, name)
    assert set(n for n, _, _ in CASES) == set(OK)
    mine = [(kw, msg) for n, kw, msg in CASES if n == name]
    assert len(mine) >= 12
    for kw, msg in mine:
        assert set(kw) <= set(OK[name]), (name, set(kw) - set(OK[name]))
        rc = fn(*{**OK[name], **kw}.values())
        if msg is None:
            assert rc == 0, (name, kw, rc, L.srx_last_error())
        else:
            err = L.srx_last_error()
            assert rc == -1 and err == f"{name}: {msg}".encode() or (rc == -1 and err.startswith(f"{name}: ".encode()) and msg.encode() in err), \
                (name, kw, rc, err)


# ---- the FieldTable doors on CPU tensors: every refusal here comes before any device call --------------------------------------------
N = 70


def _table(doc_base=1000):
    cols = fields.host_columns({"parent": np.arange(N, dtype=np.int64), "year": np.arange(N, dtype=np.int32), "price": np.ones(N, np.float32),
                                "tags": [["x"], ["y"]] * (N // 2), "src": ["a", "b"] * (N // 2)})
    tensors = {name: (torch.from_numpy(c.data), None) for name, c in cols.items()}
    return fields.FieldTable(cols, tensors, torch.device("cpu"), doc_base)


def _cpu_filter(t, n_filters=2):
    return DocFilter(torch.zeros((n_filters, 4), dtype=torch.int32), t.n_docs, t.doc_base)


def _raises(msg, fn, *a, **kw):
    with pytest.raises(ValueError) as e:
        fn(*a, **kw)
    assert msg in str(e.value), (msg, str(e.value))


DOC, SCORE = torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 3), dtype=torch.float32)
BAD_COUNT = torch.zeros(3, dtype=torch.int32)
BOOST_SPEC = {"functions": [{"curve": {"field": "year", "origin": 0, "step": 1, "knots": [1.0, 0.5]}}]}


def _list_doors(t):
    """(name, a call of the device door with (doc, score, count, k))"""
    return [("collapse_device", lambda d, s, c, k: t.collapse_device("parent", d, s, c, k)),
            ("sort_lists_device", lambda d, s, c, k: t.sort_lists_device("year", d, s, c, k)),
            ("facet_lists_device", lambda d, s, c, k: t.facet_lists_device("src", d, c))]


def test_device_list_triple_of_every_door():
    t = _table()
    for name, door in _list_doors(t):
        _raises(f"{name}: doc must be an int32 tensor [nq, m", door, DOC.long(), SCORE, None, 2)
        _raises(f"{name}: doc must be an int32 tensor [nq, m", door, DOC.long(), SCORE, BAD_COUNT, 9)      # two faults: doc first
        _raises(f"{name}: count must be an int32 tensor [nq]", door, DOC, SCORE, BAD_COUNT, 9)             # the count before k
        _raises(f"{name}: count must be an int32 tensor [nq]", door, DOC, SCORE, BAD_COUNT.to("meta"), 2)  # the dtype and shape before the device
        _raises(f"{name}: doc is on meta, the table on cpu", door, DOC.to("meta"), SCORE, None, 2)
        _raises(f"{name}: count is on meta, the table on cpu", door, DOC, SCORE, torch.zeros(2, dtype=torch.int32, device="meta"), 9)
        if name == "facet_lists_device":
            _raises(f"{name}: doc must be an int32 tensor [nq, m >= 1]", door, DOC[:, :0], SCORE, None, 2)
            continue
        cap = 2048
        deep = torch.zeros((1, cap + 1), dtype=torch.int32)
        _raises(f"{name} takes lists of 1 to {cap} positions, got {cap + 1} (no silent truncation)", door, deep, SCORE, None, 2)  # the depth before the score
        _raises(f"{name} takes lists of 1 to {cap} positions, got 0 (no silent truncation)", door, DOC[:, :0], SCORE, None, 2)
        _raises(f"{name}: score must be a float32 tensor of doc's shape", door, DOC, SCORE.double(), BAD_COUNT, 2)  # the score before the count
        _raises(f"{name}: score must be a float32 tensor of doc's shape", door, DOC, SCORE[:, :2], None, 9)
        _raises(f"{name}: score is on meta, the table on cpu", door, DOC, SCORE.to("meta"), None, 9)       # the device before k
        for k in (0, 4):
            _raises(f"{name}: k must be in [1, m = 3], got {k}", door, DOC, SCORE, None, k)


def test_column_and_closed_table_of_every_door():
    t = _table()
    flt = _cpu_filter(t)
    doors = [("collapse_device", lambda c: t.collapse_device(c, DOC, SCORE, None, 2)), ("collapse", lambda c: t.collapse(c, DOC.numpy(), SCORE.numpy(), None, 2)),
             ("sort_lists_device", lambda c: t.sort_lists_device(c, DOC, SCORE, None, 2)), ("sort_lists", lambda c: t.sort_lists(c, DOC.numpy(), SCORE.numpy(), None, 2)),
             ("facet_device", lambda c: t.facet_device(c, None, flt)), ("facet", lambda c: t.facet(c, None, flt)),
             ("facet_lists_device", lambda c: t.facet_lists_device(c, DOC, None)), ("facet_lists", lambda c: t.facet_lists(c, DOC.numpy())),
             ("top_by_device", lambda c: t.top_by_device(c, 2, filter=flt)), ("top_by", lambda c: t.top_by(c, 2, filter=flt)),
             ("filter_device", lambda c: t.filter_device(torch.zeros((1, 3), dtype=torch.int64), columns=[c], all=(DOC[0], DOC[0]))),
             ("boost_device", lambda c: t.boost_device([c], torch.zeros((1, 40), dtype=torch.uint8), torch.zeros(2), 0, 0, DOC, SCORE, None, 2))]
    for name, door in doors:
        _raises("unknown field 'nope'", door, "nope")
    # an unknown column wins over a bad tensor and a bad k
    _raises("unknown field 'nope'", t.collapse_device, "nope", DOC.long(), SCORE, None, 9)
    _raises("unknown field 'nope'", t.sort_lists_device, "nope", DOC.long(), SCORE, None, 9)
    _raises("unknown field 'nope'", t.facet_lists_device, "nope", DOC.long(), None)
    _raises("unknown field 'nope'", t.top_by_device, "nope", 0, q_filter=DOC[0])
    _raises("'tags' is a set column", t.collapse_device, "tags", DOC.long(), SCORE, None, 9)
    _raises("'tags' is a set column", t.sort_lists_device, "tags", DOC.long(), SCORE, None, 9)
    _raises("'tags' is a set column: a label set is no number to boost by", t.boost_device, ["year", "tags"], None, None, 0, 0, DOC, SCORE, None, 2)
    _raises("a boost takes 1 to 8 columns, got 9", t.boost_device, ["nope"] * 9, None, None, 0, 0, DOC, SCORE, None, 2)
    t.close()
    closed = "src"  # a category column: every door takes it but the boost, which takes "year"
    for name, door in doors:
        if name in ("collapse", "sort_lists", "facet", "facet_lists", "top_by"):
            continue  # the host doors upload first
        _raises("the table is closed", door, "year" if name == "boost_device" else closed)
    # the table is closed wins over a bad tensor, a bad k and a bad filter; the keywords win over the closed table
    _raises("the table is closed", t.collapse_device, "parent", DOC.long(), SCORE, None, 9)
    _raises("the table is closed", t.sort_lists_device, "parent", DOC.long(), SCORE, None, 9)
    _raises("the table is closed", t.facet_lists_device, "src", DOC.long(), None)
    _raises("the table is closed", t.facet_device, "src", None, "no filter")
    _raises("the table is closed", t.top_by_device, "year", 0, filter="no filter")
    _raises("per_group must be an integer", t.collapse_device, "parent", DOC, SCORE, None, 2, per_group=0)
    _raises("order must be one of", t.sort_lists_device, "parent", DOC, SCORE, None, 2, order="up")
    _raises("unknown field 'nope'", t.facet_device, "nope")


def test_filter_rows_resolution_of_facet_and_top_by():
    t = _table()
    flt, other = _cpu_filter(t, 2), DocFilter(torch.zeros((2, 4), dtype=torch.int32), t.n_docs, t.doc_base + 1)
    qf = torch.zeros(3, dtype=torch.int32)
    for door in (lambda **kw: t.facet_device("src", None, **kw), lambda **kw: t.top_by_device("year", 2, **kw)):
        _raises("q_filter picks rows of a filter: it needs filter=", door, q_filter=qf)
        _raises("q_filter picks rows of a filter: it needs filter=", door, q_filter=qf, n_rows=-1)      # before n_rows
        _raises("filter must be a DocFilter", door, filter="rows", n_rows=-1)
        with pytest.raises(ValueError):
            door(filter=other)                                                                           # for_index: another doc_base
        _raises("n_rows = 3 exceeds the filter's 2 rows: give q_filter", door, filter=flt, n_rows=3)
        _raises("n_rows must be >= 0", door, filter=_cpu_filter(t, 1), n_rows=-1)
        _raises("n_rows must be >= 0", door, n_rows=-1)
    # top_by_device: k before the filter, the filter before the cursor
    _raises("top_by_device: k must be in [1, 1024], got 0 (page with after=)", t.top_by_device, "year", 0, q_filter=qf)
    _raises("top_by_device: k must be in [1, 1024], got 1025 (page with after=)", t.top_by_device, "year", 1025, filter="rows")
    _raises("n_rows = 3 exceeds the filter's 2 rows", t.top_by_device, "year", 2, filter=flt, n_rows=3, after=qf.long())
    _raises("top_by_device: after must be an int32 tensor [n_rows] on cpu", t.top_by_device, "year", 2, filter=flt, after=qf)
    _raises("top_by_device: after must be an int32 tensor [n_rows] on cpu", t.top_by_device, "year", 2, filter=flt, after=qf[:2].long())


def test_host_q_filter_of_facet_and_top_by():
    t = _table()
    flt = _cpu_filter(t, 2)
    for door in (lambda **kw: t.facet("src", None, **kw), lambda **kw: t.top_by("year", 2, **kw)):
        _raises("q_filter picks rows of a filter: it needs filter=", door, q_filter=[0, 1])
        _raises("q_filter picks rows of a filter: it needs filter=", door, filter="rows", q_filter=[0, 1])  # before "filter must be a DocFilter"
        for bad in ([0, 2], [-2], [[0, 1]], [0.5]):
            with pytest.raises(ValueError, match="q_filter"):
                door(filter=flt, q_filter=bad)
    _raises("order must be one of", t.top_by, "year", 2, order="up", q_filter=[0])                            # the keywords first
    _raises("q_filter picks rows of a filter", t.top_by, "year", 2, q_filter=[0], after=[[1]])               # q_filter before after
    _raises("after must be a 1-D sequence of int32 doc ids", t.top_by, "year", 2, filter=flt, q_filter=[0, 1], after=[[1]])
    _raises("after must be a 1-D sequence of int32 doc ids", t.top_by, "year", 0, after=[2 ** 31])           # after before k


def test_host_list_door_of_every_door():
    t = _table()
    d, s = DOC.numpy(), SCORE.numpy()
    deep = np.zeros((1, 2049), np.int32)
    doors = [("collapse", 2048, lambda d, s, c, k: t.collapse("parent", d, s, c, k)), ("sort_lists", 2048, lambda d, s, c, k: t.sort_lists("year", d, s, c, k)),
             ("facet_lists", None, lambda d, s, c, k: t.facet_lists("src", d, c)), ("boost", 2048, lambda d, s, c, k: t.boost(BOOST_SPEC, d, s, c, k))]
    for name, cap, door in doors:
        with pytest.raises(ValueError):
            door(d.astype(np.float32), s, None, 2)                       # validate_candidates: ids are integers
        with pytest.raises(ValueError):
            door(d[0], s[0], None, 2)                                    # ... in two dimensions
        with pytest.raises(ValueError) as e1:
            door(d, s, [1, 2, 3], 2)                                     # ... with one count per list
        with pytest.raises(ValueError) as e2:
            door(d, s[:, :2], [1, 2, 3], 9)                              # two faults: the candidates before the score's shape
        assert str(e1.value) == str(e2.value)
        if cap is None:
            continue
        what = "the score must have doc's shape" if name == "boost" else "score must have doc's shape"
        _raises(what, door, d, s[:, :2], None, 9)                        # the score before k
        msg = (f"boost takes lists of at most {cap} positions, carry included (no silent truncation)" if name == "boost"
               else f"{name} takes lists of at most {cap} positions, got {cap + 1} (no silent truncation)")
        if name == "boost":
            _raises(what, door, deep, s[:, :2], None, 9)                 # boost: the score's shape before the cap ...
            _raises(msg, door, deep, np.zeros((1, 2049), np.float32), None, 9)
        else:
            _raises(msg, door, deep, s[:, :2], None, 9)                  # ... the others: the cap before the score's shape
    _raises("the carry's score must have doc's shape", t.boost, BOOST_SPEC, d, s, None, 2, carry=(d, s[:, :2]))
    _raises("boost takes lists of at most 2048 positions, carry included", t.boost, BOOST_SPEC, d, s, None, 2, carry=(np.zeros((2, 2046), np.int32), s[:, :2]))
    # the keywords come first
    _raises("per_group must be an integer", t.collapse, "parent", d[0], s, None, 2, per_group=0)
    _raises("nulls must be one of", t.sort_lists, "year", d[0], s, None, 2, nulls="keep")
    _raises("unknown field 'nope'", t.facet_lists, "nope", d[0])


def test_boost_device_tensors():
    t = _table()
    cl, kn = torch.zeros((1, 40), dtype=torch.uint8), torch.zeros(2)
    door = lambda d, s, c, k, **kw: t.boost_device(["year"], cl, kn, 0, 0, d, s, c, k, **kw)
    _raises("boost_device: clauses must be", t.boost_device, ["year"], cl.int(), kn, 0, 0, DOC.long(), SCORE, None, 9)  # the clauses before the lists
    _raises("boost_device: clauses must be uint8 [1 .. 8, 40]", t.boost_device, ["year"], cl[:, :39], kn.double(), 0, 0, DOC, SCORE, None, 2)
    _raises("boost_device: knots must be", t.boost_device, ["year"], cl, kn.double(), 0, 0, DOC.long(), SCORE, None, 2)
    _raises("boost_device: knots must hold 2 to 2^24 entries", t.boost_device, ["year"], cl, kn[:1], 0, 0, DOC.long(), SCORE, None, 2)
    _raises("boost_device: doc must be", door, DOC.long(), SCORE[:, :2], BAD_COUNT, 9)
    _raises("boost_device: score must be", door, DOC, SCORE[:, :2], BAD_COUNT, 9)
    _raises("boost_device: count must be", door, DOC, SCORE, BAD_COUNT, 9)
    _raises("boost_device: doc is on meta, the table on cpu", door, DOC.to("meta"), SCORE, None, 9)
    _raises("boost_device: score is on meta, the table on cpu", door, DOC, SCORE.to("meta"), None, 9)
    _raises("boost_device: carry doc must be", door, DOC, SCORE, None, 9, carry=(DOC.long(), SCORE))
    _raises("boost_device: carry doc must be int32 [nq, kc >= 1]", door, DOC, SCORE, None, 9, carry=(DOC[:1], SCORE))
    _raises("boost_device: carry score must be", door, DOC, SCORE, None, 9, carry=(DOC, SCORE[:, :2]))
    _raises("boost_device: carry count must be", door, DOC, SCORE, None, 9, carry=(DOC, SCORE, BAD_COUNT))
    deep = torch.zeros((2, 2046), dtype=torch.int32)
    _raises("boost_device takes lists of 1 to 2048 positions, carry included, got 3 + 2046 (no silent truncation)", door, DOC, SCORE, None, 0,
            carry=(deep, deep.float()))
    _raises("boost_device takes lists of 1 to 2048 positions, carry included, got 0 + 0", door, DOC[:, :0], SCORE[:, :0], None, 0)
    for k, kw, top in ((0, {}, 3), (4, {}, 3), (7, dict(carry=(DOC, SCORE)), 6)):
        _raises(f"boost_device: k must be in [1, m + kc = {top}], got {k}", door, DOC, SCORE, None, k, **kw)
