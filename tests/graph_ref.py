"""NumPy restatement of include/graph/sparse_rx_graph.h: the beam walk over a score matrix, the rank-rule prune, the reverse-edge
merge.  Plain loops: this is the statement the kernels are held to, not a fast path."""
import numpy as np


def search(V, graph, itopk, width, max_iter, k, seeds=None, n_seed=None, doc_base=0, allowed=None, score_offset=0.0):
    """V f32[nq, n_docs]: the scorer's bits; seeds i32[nq, n_seed] global ids or None (n_seed spread rows) -> (doc, score, count, stat)"""
    nq, n = V.shape
    doc = np.full((nq, k), -1, np.int32)
    score = np.zeros((nq, k), np.float32)
    count = np.zeros(nq, np.int32)
    stat = np.zeros((nq, 2), np.int32)
    for q in range(nq):
        v = (V[q] + np.float32(score_offset)).astype(np.float32)
        if seeds is None:
            first = [j * n // n_seed for j in range(n_seed)]
        else:
            first = [int(s) - doc_base for s in seeds[q]]
        visited, expanded = set(), set()

        def absorb(beam, ids):
            new = []
            for d in ids:
                if 0 <= d < n and d not in visited:
                    visited.add(d)
                    new.append(d)
            return sorted(beam + new, key=lambda d: (-v[d], d))[:itopk]

        beam = absorb([], first)
        steps = 0
        for _ in range(max_iter):
            parents = [d for d in beam if d not in expanded][:width]
            if not parents:
                break
            steps += 1
            expanded.update(parents)
            beam = absorb(beam, [int(x) for p in parents for x in graph[p]])
        keep = [d for d in beam if v[d] > 0 and (allowed is None or allowed[q, d])][:k]
        doc[q, : len(keep)] = np.asarray(keep, np.int64) + doc_base
        score[q, : len(keep)] = v[keep]
        count[q], stat[q] = len(keep), (steps, len(visited))
    return doc, score, count, stat


def _valid_positions(row, x, n):
    seen, out = set(), []
    for j, y in enumerate(row):
        y = int(y)
        if 0 <= y < n and y != x and y not in seen:
            seen.add(y)
            out.append(j)
    return out


def prune(knn, degree):
    n, d0 = knn.shape
    out = np.full((n, degree), -1, np.int32)
    r = np.arange(d0)
    for x in range(n):
        vi = np.asarray(_valid_positions(knn[x], x, n), np.int64)
        if len(vi) == 0:
            continue
        pos_of = np.full(n, -1, np.int64)  # id -> its valid position in row x
        pos_of[knn[x, vi]] = vi
        rows = knn[knn[x, vi]]             # [valid i, r]
        J = np.where((rows >= 0) & (rows < n), pos_of[np.clip(rows, 0, n - 1)], -1)  # the position j of knn[y_i][r] in row x
        hit = (J > vi[:, None]) & (r[None, :] < J)                                  # i < j and r < j
        pairs = np.unique(np.nonzero(hit)[0] * d0 + J[hit])                          # each i counts once per j
        detours = np.bincount(pairs % d0, minlength=d0)
        keep = [knn[x, j] for j in sorted(vi, key=lambda j: (detours[j], j))[:degree]]
        out[x, : len(keep)] = keep
    return out


def merge(fwd):
    n, degree = fwd.shape
    half = degree // 2
    rev = [[] for _ in range(n)]
    for j in range(degree):  # (position, source) order
        for x in range(n):
            if 0 <= fwd[x, j] < n:
                rev[fwd[x, j]].append(x)
    out = np.full((n, degree), -1, np.int32)
    for y in range(n):
        seq = list(fwd[y, :half]) + rev[y][:half] + list(fwd[y, half:])
        keep = [seq[j] for j in _valid_positions(seq, y, n)][:degree]
        out[y, : len(keep)] = keep
    return out
