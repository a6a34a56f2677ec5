"""The driver's contract for bench.py, checked on a small batch: ONE JSON line with the metric / config fields; with --full also `roofline`'s
request-rate fields measured in the run, `cpu_baseline`, and the sub-records; a plain run measures the headline alone and can dump its outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_json_line_with_roofline_and_cpu_baseline():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--streams", "3072", "--steps", "2", "--warmup", "1", "--check-streams", "64", "--full"],
                       capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                "roofline", "cpu_baseline", "bit_exact", "kernel_ms", "byte_order", "table_placement", "untimed_passes"):
        assert key in d, key
    assert d["metric"].startswith("MB/s encode+decode per GPU") and d["unit"] == "MB/s" and d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["data"] == "synthetic" and d["bit_exact"] is True
    assert d["config"]["workload"].startswith("BASELINE configs[1]") and d["config"]["streams_per_gpu"] == 3072
    assert abs(d["value"] - 3072 * 65536 / 1e6 / (d["ms_per_step"] / 1e3)) < 0.01 * d["value"]
    rf = d["roofline"]
    for key in ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "replay_ms", "request_frac", "bound_detail"):
        assert key in rf, key
    assert rf["bound"] == "hbm" and rf["peak"] == 8000.0 and rf["unit"] == "GB/s" and "lit_decode2_kernel" in rf["kernel"]
    assert 0 < rf["replay_ms"] and 0 < rf["request_frac"] < 1.5 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-6
    assert abs(rf["request_frac"] - rf["replay_ms"] / d["kernel_ms"][rf["kernel"]]) < 1e-3
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb
    assert d["byte_order"]["mode"].startswith("learned") and d["byte_order"]["in_use"] is True
    for sub in ("mixing", "simple_binary", "decode_only"):
        s = d["configs"][sub]
        assert s["bit_exact"] is True and s["value"] > 0 and "roofline" in s and "replay_ms" in s["roofline"], sub
    assert "cpu_baseline" in d["configs"]["mixing"] and "cpu_baseline" in d["configs"]["decode_only"]


def test_plain_bench_times_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """no --full: the headline line without the host-core baseline, the replay and the sub-records; --steps is the number of timed
    steps; --dump-outputs writes the last timed step's outputs, and a second run with the same arguments writes the same arrays"""
    dumps = []
    for run in range(2):
        out = tmp_path / f"dump{run}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--streams", "2048", "--steps", "3", "--warmup", "1", "--check-streams", "64",
                            "--dump-outputs", str(out)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.strip()]
        assert len(lines) == 1, lines
        d = json.loads(lines[0])
        assert d["metric"].startswith("MB/s encode+decode per GPU") and d["unit"] == "MB/s" and d["higher_is_better"] is True
        assert d["dtype"] == "u16/u64 integer" and d["steps"] == 3 and d["bit_exact"] is True
        assert abs(d["value"] - 2048 * 65536 / 1e6 / (d["ms_per_step"] / 1e3)) < 0.01 * d["value"]
        assert "cpu_baseline" not in d and "configs" not in d and "replay_ms" not in d["roofline"]
        arrays = {f.stem: np.load(f) for f in out.glob("*.npy")}
        assert set(arrays) == {"sizes", "packed_offsets", "packed_total", "coded_sample", "decoded_sample"}
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        assert sum(f.stat().st_size for f in out.glob("*.npy")) <= 64 << 20
        assert arrays["sizes"].shape == (2048,) and arrays["decoded_sample"].shape[1] == 65536
        assert abs(arrays["sizes"].sum() / (2048 * 65536) - d["compressed_ratio"]) < 1e-3
        dumps.append(arrays)
    for name, a in dumps[0].items():
        assert np.array_equal(a, dumps[1][name]), name
