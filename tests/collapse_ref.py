"""Restatement of include/sparse_rx_collapse.h in plain Python over NumPy arrays: Python ints for the keys, one loop over the
positions of a list.  It never imports the engine."""
import numpy as np

NULL_OWN, NULL_ONE, NULL_DROP = 0, 1, 2
POLICY = {"own": NULL_OWN, "one": NULL_ONE, "drop": NULL_DROP}
MAX_M = 2048


def collapse_list(keys, valid, n_docs, doc_base, doc, score_bits, count, k, per_group, policy):
    """One list.  keys: sequence of n_docs ints; valid: sequence of n_docs bools or None; doc: m ints (GLOBAL ids); score_bits: m
    uint32; count: int or None.  Returns (docs, score_bits, positions, group_sizes) of the first k survivors."""
    m = len(doc)
    live_prefix = m if count is None else min(max(int(count), 0), m)
    group_of = [None] * m  # None: in no group (dead or dropped)
    for c in range(live_prefix):
        local = int(doc[c]) - int(doc_base)
        if not (0 <= local < n_docs):
            continue
        if valid is None or bool(valid[local]):
            group_of[c] = ("key", int(keys[local]))
        elif policy == NULL_OWN:
            group_of[c] = ("own", c)
        elif policy == NULL_ONE:
            group_of[c] = ("null",)
    size = {}
    for g in group_of:
        if g is not None:
            size[g] = size.get(g, 0) + 1
    seen = {}
    out = []
    for c in range(m):
        g = group_of[c]
        if g is None:
            continue
        earlier = seen.get(g, 0)
        seen[g] = earlier + 1
        if earlier < per_group and len(out) < k:
            out.append((int(doc[c]), int(score_bits[c]), c, size[g]))
    return out


def collapse(keys, valid, n_docs, doc_base, cand_doc, cand_score, cand_count, k, per_group=1, policy=NULL_OWN):
    """The whole call: cand_doc i32[nq, m], cand_score f32[nq, m], cand_count i32[nq] or None -> (out_doc i32[nq, k], out_score
    f32[nq, k], out_count i32[nq], out_pos i32[nq, k], out_group_size i32[nq, k]), padded with -1 / +0.0f / -1 / 0."""
    cand_doc = np.asarray(cand_doc)
    nq, m = cand_doc.shape
    assert 1 <= m <= MAX_M and 1 <= k <= m and per_group >= 1 and policy in (NULL_OWN, NULL_ONE, NULL_DROP)
    bits = np.ascontiguousarray(cand_score, dtype=np.float32).view(np.uint32).reshape(nq, m)
    keys = [int(x) for x in keys]
    valid = None if valid is None else [bool(x) for x in valid]
    out_doc = np.full((nq, k), -1, np.int32)
    out_bits = np.zeros((nq, k), np.uint32)
    out_count = np.zeros(nq, np.int32)
    out_pos = np.full((nq, k), -1, np.int32)
    out_size = np.zeros((nq, k), np.int32)
    for q in range(nq):
        rows = collapse_list(keys, valid, n_docs, doc_base, cand_doc[q], bits[q], None if cand_count is None else cand_count[q], k, per_group, policy)
        out_count[q] = len(rows)
        for t, (d, b, p, g) in enumerate(rows):
            out_doc[q, t], out_bits[q, t], out_pos[q, t], out_size[q, t] = d, b, p, g
    return out_doc, out_bits.view(np.float32), out_count, out_pos, out_size
