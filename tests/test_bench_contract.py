"""bench.py's output contract, checked end to end on a small instance of the same workload (GPU): one JSON line with the keys the
driver reads, a roofline object for the dominant kernel and (--full) a cpu_baseline object timed in the same run; a plain run leaves the
--full legs out, and --dump-outputs writes the last timed step's results, the same arrays from run to run."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = {"tids": np.float64, "distances": np.float32, "element_ids": np.float64, "counts": np.float64, "query_rows": np.float64}


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _load_dump(d):
    out = {}
    for name, dt in DUMPED.items():
        a = np.load(os.path.join(d, name + ".npy"))
        assert a.dtype == dt, (name, a.dtype)
        out[name] = a
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= 64 << 20
    return out


def test_dump_outputs_samples_past_the_cap(tmp_path, monkeypatch):
    """Past the size cap the dump is a fixed, seeded sample of the queries, named by query_rows.npy; below it, every query."""
    b = _bench_module()
    monkeypatch.setattr(b, "DUMP_MAX_BYTES", 1 << 16)
    nq, k = 2000, 10
    rng = np.random.default_rng(3)
    res = (rng.integers(0, 1 << 40, (nq, k)), rng.random((nq, k), dtype=np.float32), rng.integers(0, 1 << 31, (nq, k)).astype(np.uint32),
           np.full(nq, k, np.uint32))
    for r in range(2):
        b.dump_outputs(str(tmp_path / str(r)), res)
    a, c = _load_dump(str(tmp_path / "0")), _load_dump(str(tmp_path / "1"))
    rows = a["query_rows"].astype(np.int64)
    assert 0 < len(rows) < nq and (np.diff(rows) > 0).all() and sum(v.nbytes for v in a.values()) <= 1 << 16
    assert all((a[n] == c[n]).all() for n in DUMPED)
    assert (a["tids"] == res[0][rows]).all() and (a["distances"] == res[1][rows]).all() and (a["element_ids"] == res[2][rows]).all()
    b.dump_outputs(str(tmp_path / "small"), tuple(x[:50] for x in res))
    assert (_load_dump(str(tmp_path / "small"))["query_rows"] == np.arange(50)).all()


@pytest.mark.gpu
def test_bench_prints_one_contract_line():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--rows", "30000", "--queries", "600",
           "--cpu-build-rows", "300", "--cpu-queries", "50", "--full"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["dtype"] == "f32" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and abs(d["value"] - 600 * 2 / (d["ms_per_step"] * 2 / 1000.0)) <= 0.01 * d["value"]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert "traffic" in r and r["launches"] == 2
    c = d["cpu_baseline"]
    assert c["kind"] == "port" and c["cores"] == 1 and c["value"] > 0 and c["unit"] == "queries/s" and "sample" in c
    assert c["all_cores"]["cores"] >= 1 and c["all_cores_vectorised"]["value"] > 0
    assert 0.5 <= d["recall_at_10"] <= 1.0 and d["build_sec"] > 0


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """Without --full: the headline keys, none of the --full legs.  --dump-outputs: the last of 3 timed steps (query batch 0 of 2) with the
    distances of the returned rows, identical in two runs with the same arguments."""
    import torch
    rows_n, nq, k = 30000, 600, 10
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--rows", str(rows_n), "--queries", str(nq)]
    dumps = []
    for r in range(2):
        d = str(tmp_path / ("run%d" % r))
        out = subprocess.run(cmd + ["--dump-outputs", d], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        lines = [l for l in out.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, lines
        j = json.loads(lines[0])
        assert j["steps"] == 3 and j["value"] > 0 and abs(j["value"] - nq * 3 / (j["ms_per_step"] * 3 / 1000.0)) <= 0.01 * j["value"]
        assert j["unit"] == "queries/s" and j["higher_is_better"] is True and j["dtype"] == "f32" and 0.5 <= j["recall_at_10"] <= 1.0
        assert j["roofline"]["launches"] == 3
        for key in ("cpu_baseline", "roofline_k1_batched_l2", "query_batch_sweep", "ef_search_sweep"):
            assert j[key] is None, key
        dumps.append(_load_dump(d))
    a, b = dumps
    for n in DUMPED:
        assert a[n].tobytes() == b[n].tobytes(), n
    assert a["tids"].shape == (nq, k) and (a["counts"] == k).all() and (a["query_rows"] == np.arange(nq)).all()
    bm = _bench_module()
    dev = torch.device("cuda", 0)
    rows, centres = bm.synth(rows_n, 768, "gmm", 11, dev)
    queries, _ = bm.synth(nq, 768, "gmm", 12, dev, centres)
    t = torch.from_numpy(a["tids"].astype(np.int64)).to(dev)
    want = ((queries[:, None, :] - rows[t]) ** 2).sum(-1).cpu().numpy()
    assert np.allclose(a["distances"], want, rtol=1e-4, atol=1e-4)
