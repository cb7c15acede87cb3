"""The Python restatement of the search planner (tests/parity.py: plan, plan_workspace_bytes, t2_grid) on hand-computed
cases.  The GPU suite (test_search_plans.py) pins the restatement to the library's own planner through
srx_search_workspace_bytes; here the bucket arithmetic itself is checked, without a GPU."""
import pytest

from parity import plan, plan_label, plan_workspace_bytes, t2_grid


def test_c3_headline_plan():
    # C3: 10 M docs, 16 384-doc tiles (611 tiles), one-tile units, 10 000 queries, k = 100, default target 3 072:
    # three whole rounds (9 216 queries) and a tail of 784 queries cut into 3072 // 784 = 3 splits each
    p = plan(611, 1, 10_000, 100)
    assert (p["n_whole"], p["tail"], p["n_splits"], p["lists_per_q"]) == (9216, 784, 3, 6)
    assert p["items"] == 9216 + 784 * 3 and p["merge_kernel"] == "wave" and p["in_kernel_merge"] and not p["t2_everything"]
    assert plan_label(p, 100) == "mixed9216+784x3-k100-merge-wave-inkernel"


@pytest.mark.parametrize("nq,n_whole,tail,ns", [(40, 32, 8, 2), (37, 32, 5, 3), (36, 32, 4, 4), (35, 32, 3, 4), (33, 32, 1, 4)])
def test_mixed_tails(nq, n_whole, tail, ns):
    p = plan(100, 4, nq, 100, target_blocks=16)  # 25 units: the unit count does not cap the splits
    assert (p["n_whole"], p["tail"], p["n_splits"]) == (n_whole, tail, ns)


def test_whole_batches():
    for nq in (16, 32, 48):  # a multiple of the target: whole rounds only, no tail, nothing split
        p = plan(100, 4, nq, 100, target_blocks=16)
        assert (p["n_whole"], p["n_splits"], p["in_kernel_merge"]) == (0, 1, False)
        # n_whole falls back to 0: the merge kernel is launched over every query (it skips the rows tier 1 finished)
        assert p["merge_kernel"] == "wave" and p["lists_per_q"] == 2
    assert plan(100, 4, 20, 100, target_blocks=16)["n_splits"] == 4
    assert plan(4, 4, 20, 100, target_blocks=16)["n_splits"] == 1  # one unit: nothing to split


def test_split_caps():
    # all queries split (nq < target): ns = target // nq, capped by the unit count and by 4096 // (2k) candidates
    assert plan(100, 4, 16, 10)["n_splits"] == 25  # 3072 // 16 = 192 -> 25 units
    assert plan(100, 4, 16, 100)["n_splits"] == 20  # 4096 // 200
    assert plan(100, 4, 16, 512, target_blocks=64)["n_splits"] == 4
    assert plan(100, 4, 16, 513, target_blocks=64)["n_splits"] == 3
    assert plan(100, 4, 16, 1024, target_blocks=64)["n_splits"] == 2
    assert plan(100, 4, 16, 1024, target_blocks=64)["merge_kernel"] == "block"


@pytest.mark.parametrize("k,target,merge", [(128, 64, "wave"), (128, 80, "block"), (64, 128, "wave"), (64, 144, "block"),
                                             (65, 112, "wave"), (65, 128, "block"), (129, 48, "block"), (112, 64, "wave")])
def test_merge_kernel_choice(k, target, merge):
    # srx_merge_wave_kernel: k <= 128 and lists_per_q * k <= 1024 (both sides of the line), otherwise srx_merge_kernel
    p = plan(100, 4, 16, k, target_blocks=target)
    assert p["merge_kernel"] == merge, (p, k, target)


def test_tier1_k_boundary():
    assert not plan(100, 4, 36, 112, target_blocks=16)["t2_everything"]
    assert plan(100, 4, 36, 112, target_blocks=16)["in_kernel_merge"]
    p = plan(100, 4, 36, 113, target_blocks=16)
    assert p["t2_everything"] and not p["in_kernel_merge"] and p["merge_kernel"] == "wave"


def test_tier2_grid():
    p = plan(100, 4, 200, 100)  # 3072 // 200 = 15 splits: 3 000 items
    assert p["items"] == 3000 and p["t2_full"] == 1024
    assert t2_grid(p, 0) == 128 and t2_grid(p, -1) == 1024 and t2_grid(p, 7) == 1024
    assert t2_grid(plan(100, 4, 200, 113), 0) == 1024  # tier 2 takes everything: always the full grid
    assert t2_grid(plan(100, 4, 100, 100, target_blocks=100), 0) == 100  # 100 items: no smaller grid to go to


def test_workspace_bytes():
    p = plan(100, 4, 40, 100, target_blocks=16)  # 32 whole + 8 x 2 splits
    lists, items = 40 * 4, 32 + 8 * 2
    assert plan_workspace_bytes(p, 40, 100) == lists * 100 * 8 + lists * 4 + items * 1 * 4 + 4 * (1 + 8) + 4 * items + 256
    # not monotone in nq: fewer queries are cut into more splits (HostBatchPipeline regrows a slot's workspace)
    assert plan_workspace_bytes(plan(100, 4, 160, 100), 160, 100) > plan_workspace_bytes(plan(100, 4, 200, 100), 200, 100)
