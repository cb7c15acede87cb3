"""The directed fusion cases of tests/test_fuse_edges_cpu.py (table, capacity and non-finite edges) on the GPU: every case
through srx_fuse_topk and srx_fuse_topk_scored, against tests/hybrid_ref.py and tests/rescore_ref.py.  Every comparison is
on doc ids, counts and fp32 score BITS of the whole padded rows; nothing here has a tolerance."""
import zlib

import numpy as np
import pytest

import hybrid_ref
import rescore_ref
import sparse_rx
from test_fuse_edges_cpu import CASES, F32, N_CASES, bits, expected_plain, get_case, plain_others

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(x):
    import torch
    return torch.as_tensor(np.array(x), device=DEV)  # a copy: the cases' arrays are read-only


def _host(triple):
    import torch
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in triple)


def _run_plain(c, run):
    mode, w, rrf_c = c.runs[run]
    return _host(sparse_rx.fuse_topk_device(tuple(_t(x) for x in c.a), tuple(_t(x) for x in c.b), c.k, mode=mode, weights=w, rrf_c=rrf_c))


def _run_scored(c, a_other, b_other, w):
    return _host(sparse_rx.fuse_scored_device(tuple(_t(x) for x in c.a), _t(a_other), tuple(_t(x) for x in c.b), _t(b_other), c.k, w))


def _assert_rows(got, exp, tag):
    """the whole padded rows: every doc word, every score word, every count"""
    assert got[0].shape == exp[0].shape and got[0].dtype == np.int32 and got[1].dtype == np.float32, tag
    print(tag, "counts", got[2].tolist(), "expected", exp[2].tolist())
    bad = np.nonzero((got[0] != exp[0]).any(axis=1) | (bits(got[1]) != bits(exp[1])).any(axis=1) | (got[2] != exp[2]))[0]
    if len(bad):
        q = int(bad[0])
        col = np.nonzero((got[0][q] != exp[0][q]) | (bits(got[1][q]) != bits(exp[1][q])))[0]
        j = int(col[0]) if len(col) else 0
        pytest.fail(f"{tag}: queries {bad.tolist()} differ; query {q} from column {j}: count {int(got[2][q])} (expected {int(exp[2][q])}), "
                    f"docs {got[0][q, j: j + 6].tolist()} (expected {exp[0][q, j: j + 6].tolist()}), "
                    f"scores {got[1][q, j: j + 6].tolist()} (expected {exp[1][q, j: j + 6].tolist()})")


def _dirty_others(name, plain):
    """what the opposite side says: the list-derived value, or -- one entry in two -- a positive value, a zero, a negative one,
    a NaN, a denormal or +inf"""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    out = []
    for p in plain:
        kind = rng.integers(0, 12, p.shape)
        o = np.array(p, F32)
        o[kind == 0] = rng.uniform(0.01, 40.0, int((kind == 0).sum()))
        o[kind == 1] = 0.0
        o[kind == 2] = -rng.uniform(0.01, 40.0, int((kind == 2).sum()))
        o[kind == 3] = np.nan
        o[kind == 4] = F32(1e-40) * rng.integers(1, 1000, int((kind == 4).sum())).astype(F32)
        o[kind == 5] = np.inf
        out.append(o)
    return out


@pytest.mark.parametrize("name", CASES)
def test_plain_fusion_on_the_directed_cases(name):
    c = get_case(name)
    assert hybrid_ref.form(c.ka, c.kb, c.k) == c.form  # the case runs in the kernel form it was written for
    for run in range(len(c.runs)):
        _assert_rows(_run_plain(c, run), expected_plain(name, run), (name, "plain") + c.runs[run])


@pytest.mark.parametrize("name", CASES)
def test_scored_fusion_on_the_directed_cases(name):
    """fed others_from_lists the scored kernel must give the restatement's rows AND the plain kernel's, on every weighted run;
    the N cases also with dirty values for what the other side says"""
    c = get_case(name)
    assert hybrid_ref.form(c.ka, c.kb, c.k) == c.form  # the dispatch rule is the plain fusion's
    a_other, b_other = plain_others(name)
    dirty = _dirty_others(name, (a_other, b_other)) if name in N_CASES else None
    assert (dirty is not None) == name.startswith("N-")
    for run, (mode, w, _) in enumerate(c.runs):
        if mode != "weighted":
            continue
        got = _run_scored(c, a_other, b_other, w)
        _assert_rows(got, rescore_ref.fuse_scored(c.a, a_other, c.b, b_other, c.k, w), (name, "scored", w))
        _assert_rows(_run_plain(c, run), got, (name, "plain kernel against scored kernel", w))
        if dirty is not None:
            _assert_rows(_run_scored(c, dirty[0], dirty[1], w), rescore_ref.fuse_scored(c.a, dirty[0], c.b, dirty[1], c.k, w),
                         (name, "scored, dirty others", w))
