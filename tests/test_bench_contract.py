"""bench.py prints ONE JSON line with the contract's fields (run small on a GPU box)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_prints_one_contract_line():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--texts", "8192", "--steps", "3", "--warmup", "1",
                        "--cpu-sample", "512"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["unit"] == "GB/s" and d["dtype"] == "u8" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1 and d["scaling"] == "weak"
    assert d["untimed_steps"] == 1 + d["config"]["settle_steps"]   # every untimed step is counted
    # `value` is the strictly serial figure; the overlapped one is an extra object
    assert d["config"]["streams"] == 1 and d["two_streams_overlapped"]["ms_per_step"] > 0
    assert abs(d["value"] - 8192 * 1024 / (d["ms_per_step"] * 1e-3) / 1e9) < 0.02 * d["value"]
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in rf, k
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, k
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["parity_on_sample"] is True
    assert d["value"] > 0 and d["ms_per_step"] > 0


def test_bench_help_needs_no_gpu():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--gpus" in r.stdout and "--steps" in r.stdout and "--dump-outputs" in r.stdout


def test_bench_refuses_zero_timed_steps():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


def test_dump_outputs_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    """dump_outputs on host tensors: whole arrays under the row budget, a fixed sorted sample over it, <= 64 MB."""
    import numpy as np
    import torch
    import bench
    assert bench.DUMP_PREFIX_ROWS * 16 + bench.DUMP_SPAN_ROWS * 24 + 4 * 128 <= 64_000_000
    monkeypatch.setattr(bench, "DUMP_SPAN_ROWS", 1000)
    n = 3000
    g = torch.Generator().manual_seed(1)
    prefix = torch.zeros(n + 1, dtype=torch.int64)
    prefix[1:] = torch.randint(0, 9, (n,), generator=g).cumsum(0)
    total = int(prefix[n])
    spans = torch.randint(0, 1 << 20, (total + 50, 2), dtype=torch.int32, generator=g)   # + unused capacity
    files = []
    for d in (tmp_path / "a", tmp_path / "b"):
        got = bench.dump_outputs(str(d), prefix, spans, n)
        assert got == {"counts_prefix": [n + 1], "spans": [1000, 2], "spans_rows": [1000]}
        files.append({f: np.load(d / (f + ".npy")) for f in got})
    a, b = files
    assert all(v.dtype == np.float64 and np.array_equal(v, b[k]) for k, v in a.items())
    rows = a["spans_rows"].astype(np.int64)
    assert rows[0] >= 0 and rows[-1] < total and (np.diff(rows) > 0).all()
    assert np.array_equal(a["spans"], spans[:total].numpy()[rows])
    assert np.array_equal(a["counts_prefix"], prefix.numpy())


@pytest.mark.gpu
def test_bench_dump_outputs_repeat_and_match_the_line(tmp_path):
    """Two runs with the same arguments dump the same outputs; they agree with the line and with --steps."""
    import numpy as np
    dumps = []
    for i, steps in enumerate((2, 5)):
        d = tmp_path / str(i)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--texts", "8192", "--steps", str(steps),
                            "--warmup", "1", "--settle", "2", "--no-cpu-baseline", "--no-overlap-leg",
                            "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == steps and line["ms_per_step"] > 0
        arrays = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
        assert set(arrays) == set(line["dump_outputs"]["arrays"]) >= {"counts_prefix", "spans"}
        assert sum(a.nbytes for a in arrays.values()) <= 64_000_000
        pre = arrays["counts_prefix"]
        assert pre.dtype == np.float64 and pre.shape == (8192 + 1,) and pre[0] == 0
        assert int(pre[-1]) == line["config"]["matches_per_batch"] > 0
        sp = arrays["spans"]
        assert sp.ndim == 2 and sp.shape[1] == 2 and (sp[:, 0] <= sp[:, 1]).all() and (sp[:, 1] <= 1024).all()
        dumps.append(arrays)
    assert dumps[0].keys() == dumps[1].keys()
    assert all(np.array_equal(v, dumps[1][k]) for k, v in dumps[0].items())
