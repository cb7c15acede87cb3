"""The bench line's contract (task statement, Measurement section), checked on the committed line of the default workload
(profiles/r03_bench_c3.log: `python bench.py` on an MI355X when every leg ran by default, `python bench.py --full` today)
-- so that a change to bench.py that drops or renames a field shows up on the CPU -- on bench.py's argument parser
(defaults: N = 1, a run of seconds), and on --dump-outputs."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line():
    with open(os.path.join(ROOT, "profiles", "r03_bench_c3.log")) as f:
        last = [l for l in f.read().splitlines() if l.startswith("{")][-1]
    return json.loads(last)


def test_committed_bench_line_has_every_contract_field():
    d = _line()
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["higher_is_better"] is True and d["vs_baseline"] is None and d["data"] == "synthetic"
    assert d["dtype"] == "f32" and d["unit"] == "queries/s" and d["scaling"] in ("strong", "weak")
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0.0 < r["frac"] < 1.0
    # value = queries of the batch / step time; achieved = algorithmic bytes / the scoring kernels' time (tier 1 + tier 2)
    assert abs(d["value"] - d["config"]["n_queries"] / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-6
    t_score = (r["kernel_ms"] + r["tier2_kernel_ms"]) * 1e-3
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / t_score / 1e9) / r["achieved"] < 1e-3
    assert t_score < d["ms_per_step"] * 1e-3  # the kernels fit inside the step the driver's clock sees
    assert r["traffic"] is None or r["traffic"] > 0.9 * r["algorithmic_bytes_per_launch"]
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0


def test_bench_defaults_are_one_gpu_and_a_short_run():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    src = open(spec.origin).read()
    assert 'add_argument("--gpus", type=int, default=1)' in src
    assert 'add_argument("--steps", type=int, default=20)' in src and 'add_argument("--warmup", type=int, default=3)' in src
    assert "oracle" in src and "reference" not in [l.strip() for l in src.splitlines() if l.strip().startswith("import ")]


@pytest.fixture
def bench_mod():
    """bench.py imported as a module (its import sets OMP_NUM_THREADS when unset: restored afterwards)."""
    saved = os.environ.get("OMP_NUM_THREADS")
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    try:
        spec.loader.exec_module(mod)
        yield mod
    finally:
        if saved is None:
            os.environ.pop("OMP_NUM_THREADS", None)
        else:
            os.environ["OMP_NUM_THREADS"] = saved


def test_bench_has_full_and_dump_options():
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert 'add_argument("--full", action="store_true"' in src
    assert 'add_argument("--dump-outputs", metavar="DIR", default=""' in src


def _rows(nq, k, seed=0):
    import torch
    rng = np.random.Generator(np.random.PCG64(seed))
    d = rng.integers(-1, 1 << 30, size=(nq, k)).astype(np.int32)
    s = rng.random((nq, k), dtype=np.float32)
    c = rng.integers(0, k + 1, size=nq).astype(np.int32)
    return d, s, c, tuple(torch.from_numpy(x) for x in (d, s, c))


def test_dump_outputs_writes_every_row_exactly(bench_mod, tmp_path):
    d, s, c, res = _rows(300, 17)
    bench_mod.dump_outputs(str(tmp_path), res)
    z = {n: np.load(tmp_path / f"{n}.npy") for n in ("doc_ids", "scores", "counts", "query_index")}
    assert z["doc_ids"].dtype == np.float64 and z["counts"].dtype == np.float64 and z["query_index"].dtype == np.float64
    assert z["scores"].dtype == np.float32
    assert np.array_equal(z["doc_ids"].astype(np.int32), d) and np.array_equal(z["counts"].astype(np.int32), c)
    assert np.array_equal(z["scores"].view(np.uint32), s.view(np.uint32))
    assert np.array_equal(z["query_index"], np.arange(300))


def test_dump_outputs_samples_a_large_batch_the_same_way_every_time(bench_mod, tmp_path):
    d, s, c, res = _rows(1000, 50, seed=1)
    cap = 100 * (50 * 12 + 16)  # room for 100 rows
    bench_mod.dump_outputs(str(tmp_path / "a"), res, max_bytes=cap)
    bench_mod.dump_outputs(str(tmp_path / "b"), res, max_bytes=cap)
    total = sum(os.path.getsize(p) for p in (tmp_path / "a").iterdir())
    assert total <= cap + 4 * 256  # + the .npy headers
    qa, qb = np.load(tmp_path / "a" / "query_index.npy"), np.load(tmp_path / "b" / "query_index.npy")
    assert len(qa) == 100 and np.array_equal(qa, qb) and np.all(np.diff(qa) > 0)
    rows = qa.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "doc_ids.npy").astype(np.int32), d[rows])
    assert np.array_equal(np.load(tmp_path / "a" / "scores.npy").view(np.uint32), s[rows].view(np.uint32))
    assert np.array_equal(np.load(tmp_path / "a" / "counts.npy").astype(np.int32), c[rows])


def _run_bench(args, timeout=600):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "bench.py")] + args
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-4000:]
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_dumps_what_the_full_run_verifies(tmp_path):
    """A small plain run and a --full run of the same arguments: the plain line carries the contract fields but none of
    the --full legs; --full checks its rows against the oracle (bit-exact, exit 3 / SystemExit otherwise); both dumps
    hold the same rows."""
    common = ["--gpus", "1", "--workload", "c2", "--docs", "250000", "--queries", "256", "--steps", "3", "--warmup", "1"]
    plain = _run_bench(common + ["--dump-outputs", str(tmp_path / "plain")])
    assert plain["steps"] == 3 and plain["ms_per_step"] > 0 and plain["unit"] == "queries/s" and plain["dtype"] == "f32"
    assert abs(plain["value"] - 256 / (plain["ms_per_step"] * 1e-3)) / plain["value"] < 1e-6
    assert plain["cpu_baseline"] is None and "parity_check" not in plain and plain["config"]["pcie_inclusive_qps"] is None
    full = _run_bench(common + ["--full", "--cpu-seconds", "2", "--dump-outputs", str(tmp_path / "full")])
    assert full["cpu_baseline"] is not None and full["parity_check"]["queries"] >= 2
    assert full["config"]["pcie_inclusive_qps"] > 0
    for n in ("doc_ids", "scores", "counts", "query_index"):
        a, b = np.load(tmp_path / "plain" / f"{n}.npy"), np.load(tmp_path / "full" / f"{n}.npy")
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), n
    assert np.load(tmp_path / "plain" / "doc_ids.npy").shape == (256, 100)
